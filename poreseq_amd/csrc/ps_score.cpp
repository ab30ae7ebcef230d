// ps_score.cpp — the edit-scoring chain of libporeseq_hip.so: ScoreMutations (cpp/MakeMutations.cpp:23-69) for several AlignData at
// once and its reductions on the device — the point-edit table, the per-group read support, the genotype likelihoods, the phase of
// het edits.  One call is
// an array of EditReq records (ps_host.h) of one EditKind; it runs as named stages over a Chain, and a call that has to be cut runs
// the same stages over sub-ranges of the same array.  The edit plans are host arithmetic in ps_editplan.h, the kernels and
// launch_score in ps_kernels.hip.  Also here: FindPointMutations and the `likes` loop of ScoreAlignments.
#include "ps_host.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace ps {

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

// FindPointMutations, cpp/FindMutations.cpp:191-234
void find_point_mutations(const Align* a, std::vector<Mut>* out) {
    point_edits(a->bases, a->states.size(), out);
    if (a->par.verbose) { fputs("Point ", stderr); fflush(stderr); }   // cpp/FindMutations.cpp:230-231
}

namespace {
// Where one AlignData's results lie on the device — the one statement of it: the descriptors point there and the copy back reads
// from there.  `score`: doubles into the score block at the head of "mutdbl" (every kind).  The others: bytes into the call's own
// output buffer ("ptable" or "support"), valid where the flag beside them is set.
struct OutAt {
    bool live = false;        // it has events and edits: the kernels have something to score
    size_t score = 0;
    bool has_best = false, has_table = false;   // Points
    size_t best = 0, table = 0;
    bool has_rec = false;                       // Support, Genotype (sscore with `live`; lik, ncover with `live` of a genotype call)
    size_t sscore = 0, rec = 0, lik = 0, ncover = 0;
    bool has_score = false, has_hap = false;    // Phase (link, phase, nsets with `live`)
    size_t link = 0, phase = 0, hap = 0, nsets = 0;
};

// the tables of all AlignData on their way into "mutint": push() appends one and answers where it will lie on the device
struct IntStage {
    int* dp = nullptr;
    std::vector<int> h;
    const int* push(const std::vector<int>& v) { const int* at = dp + h.size(); h.insert(h.end(), v.begin(), v.end()); return at; }
};

// one call, or one sub-batch of it, on its way through the stages below, which fill it in this order
struct Chain {
    Runtime* rt;
    EditKind kind;
    EditReq* r;    // r[0 .. R - 1]
    int R;
    Tick tk;
    bool sparse = false;   // kept columns (strip sweeps) instead of full matrices
    int njobs_all = 0, extra = 0;
    double sparse_bytes = 0;
    std::vector<const int*> d_keep;   // [2 * region + direction]
    std::vector<JobSpec> specs;
    std::vector<int> job0;
    Batch b;
    SlabHold slab;   // (released at every return)
    std::vector<OutAt> at;
    size_t score_tot = 0, out_bytes = 0;
    double* score0 = nullptr;   // the score block on the device
    char* d_out = nullptr;      // the output buffer of a point-table / support / genotype call
    ScoreLaunch L;
    static const char* name(EditKind k) {
        return k == EditKind::Points ? "point_table" : k == EditKind::Phase ? "score_mutation_phase" : k == EditKind::Genotype ? "score_mutation_genotypes" : k == EditKind::Support ? "score_mutation_support" : "score_mutations";
    }
    Chain(Runtime* rt_, EditKind kind_, EditReq* r_, size_t n) : rt(rt_), kind(kind_), r(r_), R((int)n), tk(name(kind_)) { L.kind = kind_; }
    bool points() const { return kind == EditKind::Points; }
    bool support() const { return kind == EditKind::Support || kind == EditKind::Genotype; }
    bool geno() const { return kind == EditKind::Genotype; }
    bool phase() const { return kind == EditKind::Phase; }
};
}  // namespace

// ---- stage: columns.  Which columns of the score matrices will the edit lists read?  A short list (FindMutations' found edits, the
// rounds of MakeMutations' recursion: tens to hundreds of edits per region) reads a few percent of them: the fills then run as strip
// sweeps that keep those columns only (ps_sweep.hip, k_sweeps) — a few MB per alignment instead of 2 x 110 MB.  A list that
// touches more than a quarter of the columns (Refine's point edits at every position) takes full matrices.
static void choose_columns(Chain& c) {
    static const double sparse_frac = getenv("PORESEQ_SPARSE_FRAC") ? atof(getenv("PORESEQ_SPARSE_FRAC")) : 0.25;
    c.sparse = sweep_enabled();
    for (int k = 0; k < c.R && c.sparse; k++) {
        const Align* a = c.r[k].a;
        EditPlan& p = c.r[k].plan;
        const int C = (int)a->states.size();
        if (p.keep[0].empty()) plan_keep(C, &p);   // (C + 2 entries once computed)
        if (std::max(p.nkeep[0], p.nkeep[1]) > sparse_frac * C) c.sparse = false;
        const int K = sweep_guess_k(a->par.realign_width);
        if (!K) c.sparse = false;
        c.njobs_all += a->E;
        for (int e = 0; e < a->E && c.sparse; e++)
            c.sparse_bytes += 1.15 * sweep_job_bytes(a->n[e], C, sweep_guess_form(a->par.realign_width, 1)) + 16.0 * (p.nkeep[0] + p.nkeep[1]) * (std::min(2 * a->par.realign_width + 1, a->n[e]) + 24);
    }
    if (c.sparse && 2 * c.njobs_all < sparse_min()) c.sparse = false;
    if (c.tk.on) {
        double fr = 0; size_t M = 0;
        for (int k = 0; k < c.R; k++) {
            const EditPlan& p = c.r[k].plan;
            M += p.M;
            if (!p.keep[0].empty()) fr = std::max(fr, (double)std::max(p.nkeep[0], p.nkeep[1]) / std::max<size_t>(c.r[k].a->states.size(), 1));
        }
        fprintf(stderr, "[ps] score_mutations: %d regions, %d events, %zu edits, kept columns <= %.3f of a matrix: %s\n", c.R, c.njobs_all, M, fr, c.sparse ? "kept columns" : "full matrices");
    }
}

// the kept-column tables of all AlignData in one block (before the jobs are built: their descriptors point into it)
static int upload_keep(Chain& c) {
    c.d_keep.assign(2 * (size_t)c.R, nullptr);
    if (!c.sparse) return PS_OK;
    size_t tot = 0;
    for (int k = 0; k < c.R; k++) tot += c.r[k].plan.keep[0].size() + c.r[k].plan.keep[1].size();
    DBuf& kb = c.rt->buf("keep");
    PS_TRY(kb.ensure(std::max<size_t>(tot, 1) * sizeof(int)));
    std::vector<int> hk;
    hk.reserve(tot);
    for (int k = 0; k < c.R; k++)
        for (int d = 0; d < 2; d++) {
            const std::vector<int>& keep = c.r[k].plan.keep[d];
            c.d_keep[2 * k + d] = kb.as<int>() + hk.size();
            hk.insert(hk.end(), keep.begin(), keep.end());
        }
    return c.rt->up(kb.p, hk.data(), hk.size() * sizeof(int));
}

// ---- stage: jobs.  Alignment::update for every event of every AlignData
static void build_jobs(Chain& c) {
    c.job0.assign(c.R, 0);
    for (int k = 0; k < c.R; k++) {
        Align* a = c.r[k].a;
        const EditPlan& p = c.r[k].plan;
        c.job0[k] = (int)c.specs.size();
        c.extra = std::max(c.extra, p.extra);
        for (int e = 0; e < a->E; e++) {
            JobSpec s = a->job(e);
            if (c.sparse) for (int d = 0; d < 2; d++) { s.keep[d] = c.d_keep[2 * k + d]; s.nkeep[d] = p.nkeep[d]; }
            c.specs.push_back(s);
        }
    }
}

// An AlignData without events has every score at its seed, -1e-6 (score_mutations): a point-table call's rows say so, a support
// call's records are all zero, a genotype call's likelihoods and covering-event counts too, and a phase call gets what its rules give
// for all-zero links: every site a set of its own.  No kernel sees it; written here.
static void write_eventless(const Chain& c) {
    for (int k = 0; k < c.R; k++) {
        const EditReq& q = c.r[k];
        if (q.a->E) continue;
        const size_t M = (size_t)q.plan.M;
        if (c.points()) point_rows_seed(q.pos_triv, q.table, q.best);
        if (c.support()) {
            if (q.score) std::fill(q.score, q.score + M, -1e-6);
            if (q.rec) memset(q.rec, 0, M * q.ngroups * sizeof(ps_edit_support));
        }
        if (c.geno()) {
            std::fill(q.lik, q.lik + M * (q.nfrac + 1), 0.0);
            if (q.ncover) std::fill(q.ncover, q.ncover + M, 0);
        }
        if (c.phase()) {
            if (q.score) std::fill(q.score, q.score + M, -1e-6);
            memset(q.link, 0, M * q.window * sizeof(ps_edit_link));
            for (size_t m = 0; m < M; m++) { q.phase[m].vote = 0.0; q.phase[m].hap = 1; q.phase[m].set = (int32_t)m; }
            if (q.nsets) *q.nsets = (int32_t)M;   // (hap has no rows)
        }
    }
}

// ---- stage: realign.  Takes the slab of a call on full matrices, builds the batch and enqueues the fills, so that they run while
// the host prepares the edit tables.  PS_SPLIT: the bands came out wider than guessed and nothing was launched.
static int take_slab_and_realign(Chain& c) {
    const int R = c.R;
    const Align* a0 = c.r[0].a;
    double lone_need = 0;   // a single AlignData cannot be split: matrices beyond a slab go to the runtime's own pools
    if (!c.sparse && R == 1) for (int e = 0; e < a0->E; e++) lone_need += matrix_bytes((int64_t)a0->n[e] + (int64_t)a0->states.size() + 1, most_slots_w(a0->par.realign_width), 2);
    if (!c.sparse && lone_need <= (double)slab_bytes()) {
        PS_TRY(slab_acquire(&c.slab));
        if (R == 1 && lone_need > (double)c.slab.bytes) {
            // the slab this call was handed is smaller than the plan (a device fuller than expected: slab_acquire's fallback sizes) and a
            // single AlignData cannot be split: its matrices go to the runtime's own pools, as those beyond a planned slab do
            c.slab.release();
        } else {
            if (c.rt->prof_on) c.rt->prof["slab"].launches++;   // (dense calls that took a slab: a host-side count)
            c.slab.drain = c.rt->stream;
            c.b.ext = c.slab.p; c.b.ext_bytes = R > 1 ? std::min(c.slab.bytes, (size_t)dense_cap_bytes()) : c.slab.bytes;
        }
        c.tk.lap("slab wait");
    }
    PS_TRY(c.b.build(c.rt, c.specs, 2, c.extra));
    return realign(c.rt, c.b, R > 1 ? (c.sparse ? PLAN_OVER_GUESS * device_share_bytes() : (double)c.b.ext_bytes) : 0.0);
}

// ---- stage: output layout.  Every AlignData's score array back to back at the head of "mutdbl": ONE device-to-host copy returns
// them all (a copy per region before: 20 000 of a bench step's 25 000 copy commands, ~0.2 ms each on a loaded stream).  A point-table
// call: the records, then the rows, of all AlignData back to back in one buffer; a support call: the scores, then the records; a
// genotype call's likelihoods and covering-event counts follow them in the same buffer; a phase call: the scores, the links, the
// phase records, the event records and the set counts — ONE copy back each.
static void lay_out(Chain& c) {
    const int R = c.R;
    c.at.assign(R, OutAt());
    size_t& n = c.out_bytes;
    auto take = [&](size_t* at, size_t bytes) { *at = n; n += bytes; };
    for (int k = 0; k < R; k++) {
        const EditReq& q = c.r[k];
        OutAt& o = c.at[k];
        o.live = q.plan.M > 0 && q.a->E > 0;
        o.score = c.score_tot; c.score_tot += (size_t)std::max(q.plan.M, 1);
        o.has_best = c.points() && q.best && q.a->E;
        o.has_table = c.points() && q.table && q.a->E;
        o.has_rec = c.support() && o.live && q.rec;
    }
    for (int k = 0; k < R; k++) if (c.at[k].has_best) take(&c.at[k].best, c.r[k].pos_triv.size() * sizeof(ps_point_best));
    for (int k = 0; k < R; k++) if (c.at[k].has_table) take(&c.at[k].table, c.r[k].pos_triv.size() * PT_SLOTS * sizeof(double));
    if (c.phase()) {
        for (int k = 0; k < R; k++) {
            const EditReq& q = c.r[k];
            OutAt& o = c.at[k];
            if (!o.live) continue;
            const size_t M = (size_t)q.plan.M;
            o.has_score = q.score != nullptr; o.has_hap = q.hap != nullptr;
            if (o.has_score) take(&o.sscore, M * sizeof(double));
            take(&o.link, M * q.window * sizeof(ps_edit_link));
            take(&o.phase, M * sizeof(ps_edit_phase));
            if (o.has_hap) take(&o.hap, (size_t)q.a->E * q.max_sets * sizeof(ps_event_hap));
            take(&o.nsets, 8);   // (one int32; the next double stays aligned)
        }
        return;
    }
    if (!c.support()) return;
    for (int k = 0; k < R; k++) if (c.at[k].live) take(&c.at[k].sscore, (size_t)c.r[k].plan.M * sizeof(double));
    for (int k = 0; k < R; k++) if (c.at[k].has_rec) take(&c.at[k].rec, (size_t)c.r[k].plan.M * c.r[k].ngroups * sizeof(ps_edit_support));
    if (!c.geno()) return;
    for (int k = 0; k < R; k++) if (c.at[k].live) take(&c.at[k].lik, (size_t)c.r[k].plan.M * (c.r[k].nfrac + 1) * sizeof(double));
    for (int k = 0; k < R; k++) if (c.at[k].live) take(&c.at[k].ncover, (size_t)c.r[k].plan.M * sizeof(int32_t));
}

// ---- stage: descriptors.  One AlignData's ScoreArgs: its tables into `st`, its arrays carved off "mutdbl" at *dd.  (The oldall
// array is zeroed from here, between the buffers' sizing and the upload: the one stream operation inside the descriptor fill.)
static int fill_score_args(Chain& c, int k, IntStage& st, double** dd) {
    const EditPlan& p = c.r[k].plan;
    const Align* a = c.r[k].a;
    ScoreArgs& sa = c.L.sas[k];
    memset(&sa, 0, sizeof(sa));
    sa.job0 = c.job0[k]; sa.njobs = a->E;
    sa.nitems_per_job = p.M; sa.ncolmax = p.ncolmax; sa.ws = a->par.scoring_width; sa.nr0 = p.nr0;
    sa.m_start = st.push(p.start); sa.m_mlen = st.push(p.mlen); sa.m_cm = st.push(p.cm); sa.m_ncol = st.push(p.ncol);
    sa.m_skip = st.push(p.skip); sa.m_oldidx = st.push(p.oldidx); sa.m_states = st.push(p.states); sa.r0 = st.push(p.r0s);
    for (int q = 0; q < SCORE_CLASSES; q++) { sa.cls_items[q] = st.push(p.cls[q]); sa.cls_count[q] = (int)p.cls[q].size(); }
    sa.old = *dd; *dd += (size_t)a->E * std::max(p.nr0, 1);
    sa.delta = *dd; *dd += (size_t)a->E * std::max(p.M, 1);
    sa.score = c.score0 + c.at[k].score;
    // edit positions on more than a quarter of the columns: column-pair maxima of ALL columns in one coalesced pass (k_oldall)
    sa.oldall_pitch = (int64_t)a->states.size() + 8;
    sa.maxS = c.b.maxS;
    sa.oldall = !c.b.sparse && (size_t)p.nr0 * 4 > a->states.size() && p.nr0 >= 256 ? *dd : nullptr;   // (k_oldall walks full matrices)
    if (sa.oldall) PS_HIP(hipMemsetAsync(sa.oldall, 0, (size_t)a->E * sa.oldall_pitch * sizeof(double), c.rt->stream));
    *dd += (size_t)a->E * sa.oldall_pitch;
    return PS_OK;
}

// the record a point-table, support or genotype call keeps beside one AlignData's ScoreArgs
static void fill_kind_args(Chain& c, int k, IntStage& st) {
    const EditReq& r = c.r[k];
    const OutAt& o = c.at[k];
    if (c.points()) {
        PointArgs& q = c.L.pts[k];
        memset(&q, 0, sizeof(q));
        q.pos_first = st.push(r.pos_first); q.pos_triv = st.push(r.pos_triv); q.npos = (int)r.pos_triv.size();
        if (o.has_table) q.table = (double*)(c.d_out + o.table);
        if (o.has_best) q.best = (ps_point_best*)(c.d_out + o.best);
        if (!q.table && !q.best) q.npos = 0;
    }
    if (c.support()) {
        SupportArgs& q = c.L.sps[k];
        memset(&q, 0, sizeof(q));
        q.group = st.push(std::vector<int>(r.group, r.group + r.a->E));
        if (o.has_rec) { q.ngroups = r.ngroups; q.score = (double*)(c.d_out + o.sscore); q.out = (ps_edit_support*)(c.d_out + o.rec); }
    }
    if (c.geno()) {
        GenoArgs& q = c.L.gts[k];
        memset(&q, 0, sizeof(q));
        q.nfrac = -1;
        if (o.live) {
            q.nfrac = r.nfrac;
            for (int i = 0; i < q.nfrac; i++) { q.f[i] = r.frac[i]; q.g[i] = 1.0 - q.f[i]; }
            if (!o.has_rec) q.score = (double*)(c.d_out + o.sscore);   // (k_support writes nothing for this AlignData)
            q.lik = (double*)(c.d_out + o.lik); q.ncover = (int*)(c.d_out + o.ncover);
        }
    }
    if (c.phase()) {
        PhaseArgs& q = c.L.phs[k];
        memset(&q, 0, sizeof(q));
        if (o.live) {
            q.W = r.window; q.S = r.max_sets; q.min_link = r.min_link;
            if (o.has_score) q.score = (double*)(c.d_out + o.sscore);
            q.link = (ps_edit_link*)(c.d_out + o.link); q.phase = (ps_edit_phase*)(c.d_out + o.phase);
            if (o.has_hap) q.hap = (ps_event_hap*)(c.d_out + o.hap);
            q.nsets = (int*)(c.d_out + o.nsets);
        }
    }
}

// the edit tables and their descriptors (ScoreArgs, behind the tables in the same buffer) in one copy
static int upload_descriptors(Chain& c, const IntStage& st) {
    ScoreLaunch& L = c.L;
    const size_t sa_at = (st.h.size() * sizeof(int) + 63) / 64 * 64;
    const size_t pt_at = (sa_at + (size_t)c.R * sizeof(ScoreArgs) + 63) / 64 * 64;   // (a point-table call: its PointArgs behind them; a phase call: its PhaseArgs)
    const size_t gt_at = (pt_at + L.sps.size() * sizeof(SupportArgs) + 63) / 64 * 64;   // (a genotype call: its GenoArgs behind the SupportArgs)
    std::vector<char> blob(std::max({pt_at + L.pts.size() * sizeof(PointArgs), gt_at + L.gts.size() * sizeof(GenoArgs), pt_at + L.phs.size() * sizeof(PhaseArgs)}));   // (PointArgs, SupportArgs or PhaseArgs: one of them)
    memcpy(blob.data(), st.h.data(), st.h.size() * sizeof(int));
    memcpy(blob.data() + sa_at, L.sas.data(), (size_t)c.R * sizeof(ScoreArgs));
    if (c.points()) memcpy(blob.data() + pt_at, L.pts.data(), L.pts.size() * sizeof(PointArgs));
    if (c.support()) memcpy(blob.data() + pt_at, L.sps.data(), L.sps.size() * sizeof(SupportArgs));
    if (c.geno()) memcpy(blob.data() + gt_at, L.gts.data(), L.gts.size() * sizeof(GenoArgs));
    if (c.phase()) memcpy(blob.data() + pt_at, L.phs.data(), L.phs.size() * sizeof(PhaseArgs));
    PS_TRY(c.rt->up(st.dp, blob.data(), blob.size()));
    const char* base = (const char*)st.dp;
    L.d_sas = (const ScoreArgs*)(base + sa_at);
    L.d_pts = c.points() ? (const PointArgs*)(base + pt_at) : nullptr;
    L.d_sps = c.support() ? (const SupportArgs*)(base + pt_at) : nullptr;
    L.d_gts = c.geno() ? (const GenoArgs*)(base + gt_at) : nullptr;
    L.d_phs = c.phase() ? (const PhaseArgs*)(base + pt_at) : nullptr;
    return PS_OK;
}

// sizes the device buffers, fills every AlignData's descriptors (c.L) and uploads the edit tables of all AlignData in one block
static int stage_descriptors(Chain& c) {
    const int R = c.R;
    size_t ints = 16, dbls = 1;
    for (int k = 0; k < R; k++) {
        const EditPlan& p = c.r[k].plan;
        const size_t E = (size_t)c.r[k].a->E;
        ints += (size_t)p.M * 7 + (size_t)p.M * p.ncolmax + p.nr0 + 16;
        if (c.points()) ints += c.r[k].pos_first.size() + c.r[k].pos_triv.size();
        if (c.support()) ints += E;
        dbls += E * std::max(p.nr0, 1) + E * std::max(p.M, 1) + std::max(p.M, 1) + E * (c.r[k].a->states.size() + 8);
    }
    DBuf& mb = c.rt->buf("mutint");
    PS_TRY(mb.ensure(ints * sizeof(int) + 128 + (size_t)R * (sizeof(ScoreArgs) + std::max({sizeof(PointArgs), sizeof(SupportArgs), sizeof(PhaseArgs)}) + sizeof(GenoArgs)) + 64));
    DBuf& db = c.rt->buf("mutdbl");
    PS_TRY(db.ensure(dbls * sizeof(double)));
    c.score0 = db.as<double>();
    double* dd = c.score0 + c.score_tot;
    if (c.points() || c.support() || c.phase()) {
        DBuf& ob = c.rt->buf(c.points() ? "ptable" : c.phase() ? "phase" : "support");
        PS_TRY(ob.ensure(std::max<size_t>(c.out_bytes, 16)));
        c.d_out = ob.as<char>();
    }
    IntStage st;
    st.dp = mb.as<int>();
    st.h.reserve(ints);
    c.L.sas.resize(R);
    c.L.pts.resize(c.points() ? R : 0);
    c.L.sps.resize(c.support() ? R : 0);
    c.L.gts.resize(c.geno() ? R : 0);
    c.L.phs.resize(c.phase() ? R : 0);
    for (int k = 0; k < R; k++) {
        PS_TRY(fill_score_args(c, k, st, &dd));
        fill_kind_args(c, k, st);
        if (!c.at[k].live) { c.L.sas[k].njobs = 0; c.L.sas[k].nitems_per_job = 0; }   // nothing to score for this AlignData: its blocks leave at once
    }
    return upload_descriptors(c, st);
}

// ---- stage: launch.  The lb tables of the new alignment, the profile's traffic model, the scoring kernels
static int launch(Chain& c) {
    PS_TRY(launch_lb(c.rt, c.b.d, 1, c.b.maxlbn));
    for (int k = 0; k < c.R && c.rt->prof_on; k++) {
        const EditPlan& p = c.r[k].plan;
        const Align* a = c.r[k].a;
        if (!c.at[k].live) continue;
        // per (event, edit) item  16(Bs+1) + 16 Br + 24(Bs+c) + 32 Br / k + 8
        double t = 0;
        const double Bs = 2.0 * c.L.sas[k].ws + 1, Br = 2.0 * a->par.realign_width + 1;
        const double kk = (double)p.M / std::max(p.nr0, 1);
        for (int i = 0; i < p.M; i++) t += 16 * (Bs + 1) + 16 * Br + 24 * (Bs + p.mlen[i] + 6) + 32 * Br / kk + 8;
        c.rt->prof["score"].bytes += t * a->E;
        c.rt->prof["score"].units += (double)p.M * a->E;
    }
    return launch_score(c.rt, c.b.d, c.L);
}

// ---- stage: fetch, one routine per kind.  The output buffer of a point-table, support or genotype call comes back in one copy
static int fetch_block(Chain& c, char** h) {
    *h = nullptr;
    if (c.out_bytes) PS_TRY(c.rt->down((void**)h, c.d_out, c.out_bytes));
    PS_HIP(hipStreamSynchronize(c.rt->stream));
    return PS_OK;
}
static int fetch_points(Chain& c) {
    char* h = nullptr;
    PS_TRY(fetch_block(c, &h));
    for (int k = 0; k < c.R; k++) {
        const EditReq& q = c.r[k];
        const size_t npos = q.pos_triv.size();
        if (!npos) continue;
        if (c.at[k].has_best) memcpy(q.best, h + c.at[k].best, npos * sizeof(ps_point_best));
        if (c.at[k].has_table) memcpy(q.table, h + c.at[k].table, npos * PT_SLOTS * sizeof(double));
    }
    return PS_OK;
}
static int fetch_support(Chain& c) {
    char* h = nullptr;
    PS_TRY(fetch_block(c, &h));
    for (int k = 0; k < c.R; k++) {
        const EditReq& q = c.r[k];
        const OutAt& o = c.at[k];
        const size_t M = (size_t)q.plan.M;
        if (!o.live) continue;
        if (q.score) memcpy(q.score, h + o.sscore, M * sizeof(double));
        if (q.rec) memcpy(q.rec, h + o.rec, M * q.ngroups * sizeof(ps_edit_support));
        if (!c.geno()) continue;
        memcpy(q.lik, h + o.lik, M * (q.nfrac + 1) * sizeof(double));
        if (q.ncover) memcpy(q.ncover, h + o.ncover, M * sizeof(int32_t));
    }
    return PS_OK;
}
static int fetch_phase(Chain& c) {
    char* h = nullptr;
    PS_TRY(fetch_block(c, &h));
    for (int k = 0; k < c.R; k++) {
        const EditReq& q = c.r[k];
        const OutAt& o = c.at[k];
        const size_t M = (size_t)q.plan.M;
        if (!o.live) continue;
        if (o.has_score) memcpy(q.score, h + o.sscore, M * sizeof(double));
        memcpy(q.link, h + o.link, M * q.window * sizeof(ps_edit_link));
        memcpy(q.phase, h + o.phase, M * sizeof(ps_edit_phase));
        if (o.has_hap) memcpy(q.hap, h + o.hap, (size_t)q.a->E * q.max_sets * sizeof(ps_event_hap));
        if (q.nsets) memcpy(q.nsets, h + o.nsets, sizeof(int32_t));
    }
    return PS_OK;
}
static int fetch_list(Chain& c) {
    std::vector<double*> dl(c.R, nullptr);
    double* all_scores = nullptr;
    PS_TRY(c.rt->down(&all_scores, c.score0, c.score_tot));
    for (int k = 0; k < c.R; k++)
        if (c.at[k].live && c.r[k].delta) PS_TRY(c.rt->down(&dl[k], c.L.sas[k].delta, (size_t)c.r[k].a->E * c.r[k].plan.M));
    PS_HIP(hipStreamSynchronize(c.rt->stream));
    for (int k = 0; k < c.R; k++) {
        const EditReq& q = c.r[k];
        if (!c.at[k].live) continue;
        for (int i = 0; i < q.plan.M; i++) (*q.out)[i].score = all_scores[c.at[k].score + i];
        if (dl[k]) memcpy(q.delta, dl[k], (size_t)q.a->E * q.plan.M * sizeof(double));
    }
    return PS_OK;
}

// The chain over r[0 .. n - 1], every list sized (plan_edits) and every output initialised — once per call: the sub-batches of a
// call that does not fit a slab or the runtime's share, and the halves of one whose bands came out wider than guessed, are
// sub-ranges of the same records and find their plans there instead of copying and sizing 80 000 edits per region again
static int run_chain(Runtime* rt, EditKind kind, EditReq* r, size_t n) {
    Chain c(rt, kind, r, n);
    // the reference's progress line under `verbose` (cpp/MakeMutations.cpp:28-32, 55-66: "Scoring (<width>)", a dot per event, a newline);
    // a lock-step call over several AlignData has no single line to write: only the single-handle call speaks
    if (n == 1 && r[0].a->par.verbose) {
        fprintf(stderr, "Scoring (%d)", (int)r[0].a->par.scoring_width);
        for (int e = 0; e < r[0].a->E; e++) fputc('.', stderr);
        fputc('\n', stderr);
        fflush(stderr);
    }
    choose_columns(c);
    c.tk.lap("edit sizes");
    auto sub = [&](size_t k0, size_t k1) { return run_chain(rt, kind, r + k0, k1 - k0); };   // regions k0 .. k1 - 1 as a call of their own
    auto need = [&](size_t k) { return share_need(r[k].a, 2); };
    if (c.sparse && n > 1 && c.sparse_bytes > device_share_bytes()) return in_halves(n, sub);
    if (!c.sparse && over_share(n, 2, need)) return in_share_chunks(n, 2, need, sub);   // sub-batches that fit a slab
    PS_TRY(upload_keep(c));
    build_jobs(c);
    write_eventless(c);
    if (c.specs.empty()) return PS_OK;
    {
        const int rc = take_slab_and_realign(c);
        if (rc == PS_SPLIT) { c.slab.release(); return in_halves(n, sub); }   // bands wider than guessed: two halves, one after the other
        PS_TRY(rc);
    }
    for (int k = 0; k < c.R; k++) r[k].a->host_refs_valid = false;
    c.tk.lap("realign enqueue");
    par_for(c.R, [&](int k) { plan_tables(r[k].a->bases, *r[k].muts, &r[k].plan, n == 1 ? 8 : (n <= 4 ? 4 : 1)); });
    c.tk.lap("edit geometry");
    lay_out(c);
    PS_TRY(stage_descriptors(c));
    c.tk.lap("upload");
    if (c.tk.on) { PS_HIP(hipStreamSynchronize(rt->stream)); }
    c.tk.lap("realign fwd+back (rest)");
    PS_TRY(launch(c));
    PS_TRY(kind == EditKind::Points ? fetch_points(c) : c.support() ? fetch_support(c) : c.phase() ? fetch_phase(c) : fetch_list(c));
    c.tk.lap("score edits");
    return PS_OK;
}

// One edit-scoring call: sizes every list, checks the arguments — here, once, for every kind — and runs the chain.
int score_edits(Runtime* rt, EditKind kind, EditReq* reqs, size_t n) {
    par_for((int)n, [&](int k) {   // (a Refine list is 80 000 edits per region: copied and sized side by side)
        EditReq& q = reqs[k];
        if (kind == EditKind::Points) {
            find_point_mutations(q.a, &q.own);
            q.muts = &q.own;
            point_layout(q.a->bases, q.a->states.size(), &q.pos_first, &q.pos_triv);
        }
        if (kind == EditKind::List) {
            *q.out = *q.muts;
            for (Mut& m : *q.out) m.score = -1e-6;
        }
        plan_edits(q.a->bases, (int)q.a->states.size(), q.a->par.scoring_width, *q.muts, &q.plan);
    });
    for (size_t k = 0; k < n; k++) {
        const int ws = reqs[k].a->par.scoring_width;
        if (ws < 0) return fail(PS_ERR_BAD_ARG, "scoring_width < 0");
        if (reqs[k].plan.bad_start) return fail(PS_ERR_BAD_ARG, "negative mutation start");
        // (a point list never trips this one: its edits insert at most one base, seven new columns)
        if (reqs[k].plan.ncolmax > 64 && ws > 511) return fail(PS_ERR_UNSUPPORTED, "edit longer than 58 bases with scoring_width > 511");
    }
    return run_chain(rt, kind, reqs, n);
}

int score_mutations(Runtime* rt, Align* a, const std::vector<Mut>& muts, std::vector<Mut>* out) {
    if (!a->E) {
        *out = muts;
        for (Mut& m : *out) m.score = -1e-6;
        for (const Mut& m : muts) if (m.start < 0) return fail(PS_ERR_BAD_ARG, "negative mutation start");
        return PS_OK;
    }
    EditReq q;
    q.a = a; q.muts = &muts; q.out = out;
    return score_edits(rt, EditKind::List, &q, 1);
}

}  // namespace ps
