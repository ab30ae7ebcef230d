// ps_score.cpp — the edit-scoring chain of libporeseq_hip.so: ScoreMutations (cpp/MakeMutations.cpp:23-69) for several AlignData at
// once and its reductions on the device — the point-edit table, the per-group read support, the genotype likelihoods, the phase of
// het edits.  One call is
// an array of EditReq records (ps_host.h) of one EditKind; it runs as named stages over a Chain, and a call that has to be cut runs
// the same stages over sub-ranges of the same array.  The edit plans are host arithmetic in ps_editplan.h, the kernels and
// launch_score in ps_edit.hip.  Also here: FindPointMutations and the `likes` loop of ScoreAlignments.
#include "ps_host.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

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
// ---- the output plan.  What a call returns besides the scored list, by name; which of them a kind has is kind_outputs()
enum Out { O_SCORE, O_BEST, O_TABLE, O_REC, O_LIK, O_NCOVER, O_LINK, O_PHASE, O_HAP, O_NSETS, O_COUNT };
// the caller's array for one of them (null: not wanted, or not of this kind) ...
void* out_host(const EditReq& q, Out o) {
    void* const h[O_COUNT] = {q.score, q.best, q.table, q.rec, q.lik, q.ncover, q.link, q.phase, q.hap, q.nsets};
    return h[o];
}
// ... and its size — the one statement of it (include/poreseq_hip.h documents the same shapes): the layout, the descriptors, the
// copy back and the values written without a kernel all come here
size_t out_bytes(const EditReq& q, Out o) {
    const size_t M = q.muts->size(), E = (size_t)q.a->E, npos = q.pos_triv.size();
    switch (o) {
    case O_SCORE: return M * sizeof(double);
    case O_BEST: return npos * sizeof(ps_point_best);
    case O_TABLE: return npos * PT_SLOTS * sizeof(double);
    case O_REC: return M * q.ngroups * sizeof(ps_edit_support);
    case O_LIK: return M * (q.nfrac + 1) * sizeof(double);
    case O_NCOVER: return M * sizeof(int32_t);
    case O_LINK: return M * q.window * sizeof(ps_edit_link);
    case O_PHASE: return M * sizeof(ps_edit_phase);
    case O_HAP: return E * q.max_sets * sizeof(ps_event_hap);
    case O_NSETS: return sizeof(int32_t);
    case O_COUNT: break;
    }
    return 0;
}
std::vector<Out> kind_outputs(EditKind kind) {
    switch (kind) {
    case EditKind::Points: return {O_BEST, O_TABLE};
    case EditKind::Support: return {O_SCORE, O_REC};
    case EditKind::Genotype: return {O_SCORE, O_REC, O_LIK, O_NCOVER};
    case EditKind::Phase: return {O_SCORE, O_LINK, O_PHASE, O_HAP, O_NSETS};
    case EditKind::List: break;
    }
    return {};
}
// Does one of its kind's outputs get a segment on the device?  `live`: the AlignData has events and edits, the kernels have
// something to score.  A point-table call's rows and records: where wanted.  The scores of a support or genotype call: always
// (k_support or k_genotype writes them, wanted or not); of a phase call: where wanted.  Support and event records: where wanted.
bool out_present(EditKind kind, const EditReq& q, bool live, Out o) {
    switch (o) {
    case O_BEST: case O_TABLE: return out_host(q, o) && q.a->E;
    case O_SCORE: return live && (kind != EditKind::Phase || q.score);
    case O_REC: case O_HAP: return live && out_host(q, o);
    default: return live;
    }
}
// Where one AlignData's results lie on the device — the one statement of it: the descriptors point there and the copy back reads
// from there.  `score`: doubles into the score block at the head of "mutdbl" (every kind).  `seg`: the outputs above, bytes into
// the call's own output buffer ("ptable", "support" or "phase"); `host` may be null where the device writes one nobody asked for.
struct OutSeg { bool on = false; void* host = nullptr; size_t bytes = 0, at = 0; };
struct OutAt {
    bool live = false;
    size_t score = 0;
    OutSeg seg[O_COUNT];
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

// Values no kernel writes, for every AlignData no kernel sees.  One without events has every score at its seed, -1e-6
// (score_mutations): a point-table call's rows say so, a support call's records are all zero, a genotype call's likelihoods and
// covering-event counts too, and a phase call gets what its rules give for all-zero links: every site a set of its own.  One with
// events and an empty list has arrays of no length to write — except a phase call's: no site, no set, and no event is tagged.
void write_unseen(EditKind kind, EditReq* r, size_t n) {
    auto zero = [](const EditReq& q, Out o) { if (void* h = out_host(q, o)) memset(h, 0, out_bytes(q, o)); };
    for (size_t k = 0; k < n; k++) {
        const EditReq& q = r[k];
        const size_t M = q.muts->size();
        if (M && q.a->E) continue;
        if (kind == EditKind::Points) { if (!q.a->E) point_rows_seed(q.pos_triv, q.table, q.best); continue; }
        if (q.score) std::fill(q.score, q.score + out_bytes(q, O_SCORE) / sizeof(double), -1e-6);
        for (Out o : {O_REC, O_LIK, O_NCOVER, O_LINK, O_HAP}) zero(q, o);
        if (q.phase) for (size_t m = 0; m < M; m++) { q.phase[m].vote = 0.0; q.phase[m].hap = 1; q.phase[m].set = (int32_t)m; }
        if (q.nsets) *q.nsets = (int32_t)M;
    }
}
}  // namespace

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
// them all (a copy per region before: 20 000 of a bench step's 25 000 copy commands, ~0.2 ms each on a loaded stream).  A call
// with outputs of its own (kind_outputs) gets them in one buffer, AlignData by AlignData, every segment on a multiple of 8 bytes —
// ONE copy back.
static void lay_out(Chain& c) {
    c.at.assign(c.R, OutAt());
    const std::vector<Out> outs = kind_outputs(c.kind);
    for (int k = 0; k < c.R; k++) {
        const EditReq& q = c.r[k];
        OutAt& o = c.at[k];
        o.live = q.plan.M > 0 && q.a->E > 0;
        o.score = c.score_tot; c.score_tot += (size_t)std::max(q.plan.M, 1);
        for (Out x : outs) {
            if (!out_present(c.kind, q, o.live, x)) continue;
            OutSeg& s = o.seg[x];
            s.on = true; s.host = out_host(q, x); s.bytes = out_bytes(q, x); s.at = c.out_bytes;
            c.out_bytes += (s.bytes + 7) / 8 * 8;
        }
    }
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

// the records a call's kind keeps beside one AlignData's ScoreArgs; their output pointers come from the plan, null where a segment is absent
static void fill_kind_args(Chain& c, int k, IntStage& st) {
    const EditReq& r = c.r[k];
    const OutAt& o = c.at[k];
    auto dev = [&](Out x) -> char* { return o.seg[x].on ? c.d_out + o.seg[x].at : nullptr; };
    if (c.kind == EditKind::Points) {
        PointArgs& q = c.L.pts[k];
        memset(&q, 0, sizeof(q));
        q.pos_first = st.push(r.pos_first); q.pos_triv = st.push(r.pos_triv); q.npos = (int)r.pos_triv.size();
        q.table = (double*)dev(O_TABLE); q.best = (ps_point_best*)dev(O_BEST);
        if (!q.table && !q.best) q.npos = 0;
    }
    if (c.kind == EditKind::Support || c.kind == EditKind::Genotype) {
        SupportArgs& q = c.L.sps[k];
        memset(&q, 0, sizeof(q));
        q.group = st.push(std::vector<int>(r.group, r.group + r.a->E));
        if (o.seg[O_REC].on) { q.ngroups = r.ngroups; q.score = (double*)dev(O_SCORE); q.out = (ps_edit_support*)dev(O_REC); }
    }
    if (c.kind == EditKind::Genotype) {
        GenoArgs& q = c.L.gts[k];
        memset(&q, 0, sizeof(q));
        q.nfrac = -1;
        if (o.live) {
            q.nfrac = r.nfrac;
            for (int i = 0; i < q.nfrac; i++) { q.f[i] = r.frac[i]; q.g[i] = 1.0 - q.f[i]; }
            if (!o.seg[O_REC].on) q.score = (double*)dev(O_SCORE);   // (k_support writes nothing for this AlignData)
            q.lik = (double*)dev(O_LIK); q.ncover = (int*)dev(O_NCOVER);
        }
    }
    if (c.kind == EditKind::Phase) {
        PhaseArgs& q = c.L.phs[k];
        memset(&q, 0, sizeof(q));
        if (o.live) {
            q.W = r.window; q.S = r.max_sets; q.min_link = r.min_link;
            q.score = (double*)dev(O_SCORE); q.link = (ps_edit_link*)dev(O_LINK); q.phase = (ps_edit_phase*)dev(O_PHASE);
            q.hap = (ps_event_hap*)dev(O_HAP); q.nsets = (int*)dev(O_NSETS);
        }
    }
}

// The record arrays of a call, sized for R AlignData: its ScoreArgs and what its kind keeps beside them — nothing (List), one array,
// or two (Genotype: SupportArgs and GenoArgs).  Per array: where it lies on the host, its bytes, and how launch_score is told where
// its copy lies on the device.
struct RecArray { const void* host; size_t bytes; std::function<void(const char*)> placed; };
template <class T> static RecArray rec_array(std::vector<T>& h, const T** d, int R) {
    h.resize(R);
    return {h.data(), (size_t)R * sizeof(T), [d](const char* at) { *d = (const T*)at; }};
}
static std::vector<RecArray> record_arrays(ScoreLaunch& L, int R) {
    std::vector<RecArray> v = {rec_array(L.sas, &L.d_sas, R)};
    if (L.kind == EditKind::Points) v.push_back(rec_array(L.pts, &L.d_pts, R));
    if (L.kind == EditKind::Support || L.kind == EditKind::Genotype) v.push_back(rec_array(L.sps, &L.d_sps, R));
    if (L.kind == EditKind::Genotype) v.push_back(rec_array(L.gts, &L.d_gts, R));
    if (L.kind == EditKind::Phase) v.push_back(rec_array(L.phs, &L.d_phs, R));
    return v;
}
static size_t align64(size_t n) { return (n + 63) / 64 * 64; }

// the edit tables and their descriptors (the record arrays, each on a multiple of 64 bytes behind the tables in the same buffer) in one copy
static int upload_descriptors(Chain& c, const IntStage& st, const std::vector<RecArray>& recs) {
    std::vector<size_t> at;
    size_t end = st.h.size() * sizeof(int);
    for (const RecArray& p : recs) { at.push_back(align64(end)); end = at.back() + p.bytes; }
    std::vector<char> blob(end);   // (sized once: the tables of a Refine-sized call are tens of MB)
    memcpy(blob.data(), st.h.data(), st.h.size() * sizeof(int));
    for (size_t i = 0; i < recs.size(); i++) memcpy(blob.data() + at[i], recs[i].host, recs[i].bytes);
    PS_TRY(c.rt->up(st.dp, blob.data(), blob.size()));
    for (size_t i = 0; i < recs.size(); i++) recs[i].placed((const char*)st.dp + at[i]);
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
        ints += c.r[k].pos_first.size() + c.r[k].pos_triv.size() + E;   // (a point-table call's position tables, a support or genotype call's group ids)
        dbls += E * std::max(p.nr0, 1) + E * std::max(p.M, 1) + std::max(p.M, 1) + E * (c.r[k].a->states.size() + 8);
    }
    const std::vector<RecArray> recs = record_arrays(c.L, R);
    size_t desc = align64(ints * sizeof(int));
    for (const RecArray& a : recs) desc += align64(a.bytes);
    DBuf& mb = c.rt->buf("mutint");
    PS_TRY(mb.ensure(desc));
    DBuf& db = c.rt->buf("mutdbl");
    PS_TRY(db.ensure(dbls * sizeof(double)));
    c.score0 = db.as<double>();
    double* dd = c.score0 + c.score_tot;
    if (DBuf* ob = c.points() ? &c.rt->buf("ptable") : c.phase() ? &c.rt->buf("phase") : c.support() ? &c.rt->buf("support") : nullptr) {
        PS_TRY(ob->ensure(std::max<size_t>(c.out_bytes, 16)));
        c.d_out = ob->as<char>();
    }
    IntStage st;
    st.dp = mb.as<int>();
    st.h.reserve(ints);
    for (int k = 0; k < R; k++) {
        PS_TRY(fill_score_args(c, k, st, &dd));
        fill_kind_args(c, k, st);
        if (!c.at[k].live) { c.L.sas[k].njobs = 0; c.L.sas[k].nitems_per_job = 0; }   // nothing to score for this AlignData: its blocks leave at once
    }
    return upload_descriptors(c, st, recs);
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

// ---- stage: fetch.  The output buffer of a call that has one comes back in one copy, and every segment of the plan that the
// caller wants goes to its array; a scored list comes back from the score block (fetch_list)
static int fetch_outputs(Chain& c) {
    char* h = nullptr;
    if (c.out_bytes) PS_TRY(c.rt->down((void**)&h, c.d_out, c.out_bytes));
    PS_HIP(hipStreamSynchronize(c.rt->stream));
    for (const OutAt& o : c.at)
        for (const OutSeg& s : o.seg)
            if (s.on && s.host) memcpy(s.host, h + s.at, s.bytes);
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
    write_unseen(kind, r, n);
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
    PS_TRY(kind == EditKind::List ? fetch_list(c) : fetch_outputs(c));
    c.tk.lap("score edits");
    return PS_OK;
}

// ---- argument checks of one AlignData of a point-table, support, genotype or phase call (`i`: its place in the call), in the order
// the C ABI reports them
static int check_groups(const EditReq& q, const std::string& who, bool need_records) {
    if (q.ngroups < 1 || q.ngroups > SUPPORT_MAX_GROUPS)
        return fail(PS_ERR_BAD_ARG, who + ": n_groups = " + std::to_string(q.ngroups) + ", allowed are 1 .. " + std::to_string(SUPPORT_MAX_GROUPS));
    if (!q.group) return fail(PS_ERR_BAD_ARG, who + ": null group array");
    if (need_records && !q.rec) return fail(PS_ERR_BAD_ARG, who + ": null support array");
    for (int e = 0; e < q.a->E; e++)
        if (q.group[e] < 0 || q.group[e] >= q.ngroups)
            return fail(PS_ERR_BAD_ARG, who + ": event " + std::to_string(e) + " has group " + std::to_string(q.group[e]) + ", n_groups = " + std::to_string(q.ngroups));
    return PS_OK;
}
static int check_request(EditKind kind, const EditReq& q, size_t i) {
    char msg[96];
    if (kind == EditKind::List) return PS_OK;   // (its callers have no ranges to check)
    if (kind == EditKind::Points) {
        const int64_t have = (int64_t)q.a->states.size();
        if (q.npos_given != have)
            return fail(PS_ERR_BAD_ARG, "ps_batch_point_table: region " + std::to_string(i) + " was given n = " + std::to_string(q.npos_given) + ", its sequence has " +
                                        std::to_string(have) + " positions (length - 4)");
        return PS_OK;
    }
    const std::string who = std::string(kind == EditKind::Support ? "ps_score_mutation_support" : kind == EditKind::Genotype ? "ps_score_mutation_genotypes" : "ps_score_mutation_phase") +
                            ": region " + std::to_string(i);
    if (!q.muts) return fail(PS_ERR_BAD_ARG, who + ": null list");
    if (kind == EditKind::Support) return check_groups(q, who, true);
    if (kind == EditKind::Genotype) {
        PS_TRY(check_groups(q, who, false));
        if (q.nfrac < 0 || q.nfrac > GENO_MAX_FRAC)
            return fail(PS_ERR_BAD_ARG, who + ": n_frac = " + std::to_string(q.nfrac) + ", allowed are 0 .. " + std::to_string(GENO_MAX_FRAC));
        if (q.nfrac > 0 && !q.frac) return fail(PS_ERR_BAD_ARG, who + ": null alt_frac with n_frac = " + std::to_string(q.nfrac));
        for (int k = 0; k < q.nfrac; k++)
            if (!(q.frac[k] >= 1e-6 && q.frac[k] <= 1.0 - 1e-6)) {   // (NaN fails both comparisons)
                snprintf(msg, sizeof msg, ": alt_frac[%d] = %g, allowed is 1e-06 .. 1 - 1e-06", k, q.frac[k]);
                return fail(PS_ERR_BAD_ARG, who + msg);
            }
        if (!q.lik) return fail(PS_ERR_BAD_ARG, who + ": null lik");
        return PS_OK;
    }
    if (q.window < 1 || q.window > LINK_MAX_WINDOW)
        return fail(PS_ERR_BAD_ARG, who + ": window = " + std::to_string(q.window) + ", allowed are 1 .. " + std::to_string(LINK_MAX_WINDOW));
    if (q.max_sets < 1 || q.max_sets > PHASE_MAX_SETS)
        return fail(PS_ERR_BAD_ARG, who + ": max_sets = " + std::to_string(q.max_sets) + ", allowed are 1 .. " + std::to_string(PHASE_MAX_SETS));
    if (!(q.min_link >= 0.0 && q.min_link <= 1.7976931348623157e308)) {   // (NaN fails both comparisons)
        snprintf(msg, sizeof msg, ": min_link = %g, allowed is a finite value >= 0", q.min_link);
        return fail(PS_ERR_BAD_ARG, who + msg);
    }
    if (!q.link) return fail(PS_ERR_BAD_ARG, who + ": null link");
    if (!q.phase) return fail(PS_ERR_BAD_ARG, who + ": null phase");
    return PS_OK;
}

// One edit-scoring call: checks the arguments — here, once, for every kind — sizes every list and runs the chain.  `rt`: the
// caller's runtime; a null one (the point-table, support, genotype and phase entry points) is taken here, and only when there is
// something for the device to do: a call without a region, or without an edit in any list, ends before that.
int score_edits(Runtime* rt, EditKind kind, EditReq* reqs, size_t n) {
    for (size_t k = 0; k < n; k++) PS_TRY(check_request(kind, reqs[k], k));
    if (!rt) {
        size_t edits = 0;
        for (size_t k = 0; k < n; k++) edits += kind == EditKind::Points ? 1 : reqs[k].muts->size();
        if (!edits) { write_unseen(kind, reqs, n); return PS_OK; }   // nothing to score anywhere: no launch
        PS_TRY(runtime(&rt));
    }
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
