// ps_api.cpp — the C ABI of include/poreseq_hip.h over the HIP implementation.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>

#include "ps_host.h"
#include "ps_sw.h"

using namespace ps;

struct ps_align { Align a; };
struct ps_muts { std::vector<Mut> v; };
struct ps_seqs { std::vector<std::string> v; };
struct ps_rng { RandState* s = nullptr; ~ps_rng() { if (s) rand_state_free(s); } };

#define NEED_RT()            \
    Runtime* rt = nullptr;   \
    PS_TRY(runtime(&rt))

extern "C" {

const char* ps_last_error(void) { return last_error(); }
const char* ps_backend_name(void) { return "hip-gfx950"; }
int ps_info(char* out, int64_t cap) {
    if (!out || cap <= 0) return fail(PS_ERR_BAD_ARG, "ps_info");
    const std::string s = info_string();
    const size_t n = std::min<size_t>(s.size(), (size_t)cap - 1);
    memcpy(out, s.data(), n);
    out[n] = 0;
    return PS_OK;
}

int ps_align_create(ps_align** out, const char* seq, int64_t seq_len, int32_t n_events,
                    const int64_t* level_off, const double* mean, const double* stdv,
                    const double* ref_align, const double* ref_like, const double* model,
                    const double* trans, const char* evseq, const int64_t* evseq_off,
                    const ps_params* params) {
    if (!out || !seq || seq_len < 0 || n_events < 0 ||
        (n_events && (!level_off || !mean || !stdv || !ref_align || !ref_like || !model || !trans)))
        return fail(PS_ERR_BAD_ARG, "ps_align_create: bad argument");
    NEED_RT();
    std::unique_ptr<ps_align> h(new ps_align());
    PS_TRY(h->a.create(rt, seq, seq_len, n_events, level_off, mean, stdv, ref_align, ref_like, model, trans,
                       evseq, evseq_off, params));
    *out = h.release();
    return PS_OK;
}
void ps_align_destroy(ps_align* a) { delete a; }
int ps_align_set_scoring_width(ps_align* a, int32_t w) {
    if (!a) return fail(PS_ERR_BAD_ARG, "null handle");
    a->a.par.scoring_width = w;
    return PS_OK;
}
int ps_align_new_call(ps_align* a, int32_t w) {
    if (!a) return fail(PS_ERR_BAD_ARG, "null handle");
    a->a.par.scoring_width = w;
    a->a.seqlikes.clear();
    if (!a->a.keep_valid || !a->a.restore_due) return PS_OK;   // (no device work unless a scoring call asked for its refs to be kept)
    NEED_RT();
    return a->a.restore_refs(rt);
}
int ps_align_keep_refs(ps_align* a) {
    if (!a) return fail(PS_ERR_BAD_ARG, "null handle");
    NEED_RT();
    return a->a.keep_refs(rt);
}
int32_t ps_align_n_events(const ps_align* a) { return a ? a->a.E : 0; }
int64_t ps_align_n_levels(const ps_align* a, int32_t e) { return (a && e >= 0 && e < a->a.E) ? a->a.n[e] : -1; }
int64_t ps_align_sequence_length(const ps_align* a) { return a ? (int64_t)a->a.bases.size() : -1; }
int ps_align_get_sequence(const ps_align* a, char* out, int64_t cap) {
    if (!a || !out || cap < (int64_t)a->a.bases.size()) return fail(PS_ERR_BAD_ARG, "ps_align_get_sequence");
    memcpy(out, a->a.bases.data(), a->a.bases.size());
    return PS_OK;
}
int ps_align_get_event_refs(const ps_align* ca, int32_t e, double* ra, double* rl) {
    ps_align* a = const_cast<ps_align*>(ca);
    if (!a || e < 0 || e >= a->a.E) return fail(PS_ERR_BAD_ARG, "ps_align_get_event_refs");
    NEED_RT();
    PS_TRY(a->a.refs_to_host(rt));
    const int64_t o = a->a.off[e];
    if (ra) memcpy(ra, a->a.h_ra.data() + o, a->a.n[e] * sizeof(double));
    if (rl) memcpy(rl, a->a.h_rl.data() + o, a->a.n[e] * sizeof(double));
    return PS_OK;
}

int ps_muts_create(ps_muts** out, int64_t n, const int32_t* start, const int64_t* oo, const char* op,
                   const int64_t* mo, const char* mp, const double* score) {
    if (!out || n < 0 || (n && (!start || !oo || !mo))) return fail(PS_ERR_BAD_ARG, "ps_muts_create");
    ps_muts* m = new ps_muts();
    m->v.resize(n);
    for (int64_t i = 0; i < n; i++) {
        m->v[i].start = start[i];
        if (oo[i + 1] > oo[i]) m->v[i].orig.assign(op + oo[i], op + oo[i + 1]);
        if (mo[i + 1] > mo[i]) m->v[i].mut.assign(mp + mo[i], mp + mo[i + 1]);
        m->v[i].score = score ? score[i] : -1e-6;
    }
    *out = m;
    return PS_OK;
}
void ps_muts_destroy(ps_muts* m) { delete m; }
int64_t ps_muts_count(const ps_muts* m) { return m ? (int64_t)m->v.size() : 0; }
int64_t ps_muts_orig_bytes(const ps_muts* m) { int64_t t = 0; if (m) for (auto& x : m->v) t += x.orig.size(); return t; }
int64_t ps_muts_mut_bytes(const ps_muts* m) { int64_t t = 0; if (m) for (auto& x : m->v) t += x.mut.size(); return t; }
int ps_muts_export(const ps_muts* m, int32_t* start, int64_t* oo, char* op, int64_t* mo, char* mp, double* score) {
    if (!m) return fail(PS_ERR_BAD_ARG, "ps_muts_export");
    int64_t a = 0, b = 0;
    for (size_t i = 0; i < m->v.size(); i++) {
        const Mut& x = m->v[i];
        if (start) start[i] = x.start;
        if (oo) oo[i] = a;
        if (mo) mo[i] = b;
        if (op) memcpy(op + a, x.orig.data(), x.orig.size());
        if (mp) memcpy(mp + b, x.mut.data(), x.mut.size());
        a += x.orig.size(); b += x.mut.size();
        if (score) score[i] = x.score;
    }
    if (oo) oo[m->v.size()] = a;
    if (mo) mo[m->v.size()] = b;
    return PS_OK;
}

void ps_seqs_destroy(ps_seqs* s) { delete s; }
int64_t ps_seqs_count(const ps_seqs* s) { return s ? (int64_t)s->v.size() : 0; }
int64_t ps_seqs_bytes(const ps_seqs* s) { int64_t t = 0; if (s) for (auto& x : s->v) t += x.size(); return t; }
int ps_seqs_export(const ps_seqs* s, int64_t* off, char* pool) {
    if (!s) return fail(PS_ERR_BAD_ARG, "ps_seqs_export");
    int64_t a = 0;
    for (size_t i = 0; i < s->v.size(); i++) {
        if (off) off[i] = a;
        if (pool) memcpy(pool + a, s->v[i].data(), s->v[i].size());
        a += s->v[i].size();
    }
    if (off) off[s->v.size()] = a;
    return PS_OK;
}

int ps_score_alignments(ps_align* a, double* scores, double* likes) {
    if (!a || (!scores && a->a.E)) return fail(PS_ERR_BAD_ARG, "ps_score_alignments");
    NEED_RT();
    OwnReq q{&a->a, scores, likes};
    return own_forward(rt, OwnKind::Score, true, &q, 1);
}
int ps_find_point_mutations(ps_align* a, ps_muts** out) {
    if (!a || !out) return fail(PS_ERR_BAD_ARG, "ps_find_point_mutations");
    ps_muts* m = new ps_muts();
    find_point_mutations(&a->a, &m->v);
    *out = m;
    return PS_OK;
}
int ps_find_mutations(ps_align* a, int32_t n, const int64_t* off, const char* pool, ps_muts** out) {
    if (!a || !out || n < 0 || (n && (!off || !pool))) return fail(PS_ERR_BAD_ARG, "ps_find_mutations");
    NEED_RT();
    std::vector<std::string> seeds;
    for (int i = 0; i < n; i++) seeds.emplace_back(pool + off[i], pool + off[i + 1]);
    std::unique_ptr<ps_muts> m(new ps_muts());
    PS_TRY(find_mutations(rt, &a->a, seeds, &m->v));
    *out = m.release();
    return PS_OK;
}
int ps_score_mutations(ps_align* a, const ps_muts* in, ps_muts** out) {
    if (!a || !in || !out) return fail(PS_ERR_BAD_ARG, "ps_score_mutations");
    NEED_RT();
    std::unique_ptr<ps_muts> m(new ps_muts());
    PS_TRY(score_mutations(rt, &a->a, in->v, &m->v));
    *out = m.release();
    return PS_OK;
}
int ps_score_mutation_deltas(ps_align* a, const ps_muts* in, double* deltas) {
    if (!a || !in || !deltas) return fail(PS_ERR_BAD_ARG, "ps_score_mutation_deltas");
    NEED_RT();
    std::vector<Mut> scored;
    EditReq q;
    q.a = &a->a; q.muts = &in->v; q.out = &scored; q.delta = deltas;
    return score_edits(rt, EditKind::List, &q, 1);
}
int ps_make_mutations(ps_align* a, const ps_muts* in, int32_t* nb) {
    if (!a || !in || !nb) return fail(PS_ERR_BAD_ARG, "ps_make_mutations");
    NEED_RT();
    int n = 0;
    PS_TRY(make_mutations(rt, &a->a, in->v, &n));
    *nb = n;
    return PS_OK;
}
int ps_viterbi_mutate(ps_align* a, int32_t nkeep, double skip, double stay, double mmin, double mmax,
                      int32_t verbose, ps_seqs** out) {
    if (!a || !out) return fail(PS_ERR_BAD_ARG, "ps_viterbi_mutate");
    std::unique_ptr<ps_seqs> s(new ps_seqs());
    VitCall call;
    call.nkeep = nkeep; call.skip = skip; call.stay = stay; call.mmin = mmin; call.mmax = mmax;
    call.who = "ps_viterbi_mutate"; call.lockstep = false;
    VitReq q;
    q.a = &a->a; q.out = &s->v;
    PS_TRY(viterbi_mutate(nullptr, call, &q, 1));
    if (verbose) {
        // the reference's progress line (cpp/Viterbi.cpp:258-259, 357-370): "Viterbi", a dot whenever the reference position passes a
        // multiple of 200, a newline.  The positions walked: from the first event's start to where no event is aligned any more —
        // counted here from the sequence length (the walk itself runs on the device)
        fputs("Viterbi", stderr);
        for (size_t k = 200; k <= a->a.bases.size(); k += 200) fputc('.', stderr);
        fputc('\n', stderr);
        fflush(stderr);
    }
    *out = s.release();
    return PS_OK;
}
// ---- lock-step batches (include/poreseq_hip.h) ----
int ps_rng_create(ps_rng** out, uint32_t seed) {
    if (!out) return fail(PS_ERR_BAD_ARG, "ps_rng_create");
    ps_rng* r = new ps_rng();
    r->s = rand_state_new(seed);
    *out = r;
    return PS_OK;
}
void ps_rng_destroy(ps_rng* r) { delete r; }
int ps_seqs_create(ps_seqs** out, int64_t n, const int64_t* off, const char* pool) {
    if (!out || n < 0 || (n && (!off || !pool))) return fail(PS_ERR_BAD_ARG, "ps_seqs_create");
    ps_seqs* s = new ps_seqs();
    for (int64_t i = 0; i < n; i++) s->v.emplace_back(pool + off[i], pool + off[i + 1]);
    *out = s;
    return PS_OK;
}
static int batch_handles(int32_t n, ps_align* const* a, std::vector<Align*>* as) {
    if (n < 0 || (n && !a)) return fail(PS_ERR_BAD_ARG, "batch: bad handle array");
    for (int i = 0; i < n; i++) {
        if (!a[i]) return fail(PS_ERR_BAD_ARG, "batch: null handle");
        for (int j = 0; j < i; j++) if (a[j] == a[i]) return fail(PS_ERR_BAD_ARG, "batch: the same handle twice");
        as->push_back(&a[i]->a);
    }
    return PS_OK;
}
int ps_batch_score_alignments(int32_t n, ps_align* const* a, double* const* scores, double* const* likes) {
    std::vector<Align*> as;
    PS_TRY(batch_handles(n, a, &as));
    if (n && !scores) return fail(PS_ERR_BAD_ARG, "ps_batch_score_alignments");
    NEED_RT();
    std::vector<OwnReq> rq(n);
    for (int i = 0; i < n; i++) {
        if (!scores[i] && as[i]->E) return fail(PS_ERR_BAD_ARG, "ps_batch_score_alignments: null scores");
        rq[i].a = as[i]; rq[i].scores = scores[i]; rq[i].likes = likes ? likes[i] : nullptr;
    }
    return own_forward(rt, OwnKind::Score, true, rq.data(), rq.size());
}
// What ps_batch_align_stats and ps_batch_kmer_stats check alike.  Per AlignData, in the order of their other checks: the output,
// and scores only with a realignment
static int stats_output(const std::string& who, const char* what, const void* out) { return out ? PS_OK : fail(PS_ERR_BAD_ARG, who + ": null " + what); }
static int stats_scores(const std::string& who, int32_t realign, double* const* scores, int i, OwnReq* q) {
    if (!scores || !scores[i]) return PS_OK;
    if (!realign) return fail(PS_ERR_BAD_ARG, who + ": scores without a realignment (realign == 0 launches no DP: scores must be NULL)");
    q->scores = scores[i];
    return PS_OK;
}
// What ps_batch_move_stats and ps_batch_posterior_stats check alike: an event with levels has an array wherever its AlignData passes them
static int stats_levels(const std::string& who, const Align* a, const void* const* x, const void* const* y) {
    for (int e = 0; e < a->E; e++)
        if (a->n[e] > 0 && ((x && !x[e]) || (y && !y[e]))) return fail(PS_ERR_BAD_ARG, who + ": null per-level array of event " + std::to_string(e));
    return PS_OK;
}
// and their end: no events anywhere launches nothing and takes no runtime (the tables of the k-mer call are all zero)
static int stats_run(OwnKind kind, int32_t realign, std::vector<OwnReq>& rq) {
    if (std::none_of(rq.begin(), rq.end(), [](const OwnReq& q) { return q.a->E > 0; })) {
        for (const OwnReq& q : rq) if (q.table) memset(q.table, 0, (size_t)q.ngroups * NS * sizeof(ps_kmer_cell));
        return PS_OK;
    }
    NEED_RT();
    return own_forward(rt, kind, realign != 0, rq.data(), rq.size());
}
int ps_batch_align_stats(int32_t n, ps_align* const* a, int32_t realign, double* const* scores, ps_event_stats* const* stats) {
    const std::string who = "ps_batch_align_stats";
    std::vector<Align*> as;
    PS_TRY(batch_handles(n, a, &as));
    if (n) PS_TRY(stats_output(who, "stats", stats));
    std::vector<OwnReq> rq(n);
    for (int i = 0; i < n; i++) {
        PS_TRY(stats_output(who, "stats", stats[i]));
        PS_TRY(stats_scores(who, realign, scores, i, &rq[i]));
        rq[i].a = as[i]; rq[i].stats = stats[i];
    }
    return stats_run(OwnKind::AlignStats, realign, rq);
}
int ps_align_stats(ps_align* a, int32_t realign, double* scores, ps_event_stats* stats) {
    if (!a) return fail(PS_ERR_BAD_ARG, "ps_align_stats: null handle");
    if (!stats) return fail(PS_ERR_BAD_ARG, "ps_align_stats: null stats");
    return ps_batch_align_stats(1, &a, realign, &scores, &stats);
}
int ps_batch_kmer_stats(int32_t n, ps_align* const* a, int32_t realign, const int32_t* const* groups, const int32_t* n_groups, double* const* scores,
                        ps_kmer_cell* const* table) {
    const std::string who = "ps_batch_kmer_stats";
    std::vector<Align*> as;
    PS_TRY(batch_handles(n, a, &as));
    if (n) { PS_TRY(stats_output(who, "table", table)); PS_TRY(stats_output(who, "n_groups", n_groups)); }
    std::vector<OwnReq> rq(n);
    for (int i = 0; i < n; i++) {
        PS_TRY(stats_output(who, "table", table[i]));
        if (n_groups[i] < 1 || n_groups[i] > PS_KMER_MAX_GROUPS)
            return fail(PS_ERR_BAD_ARG, who + ": n_groups = " + std::to_string(n_groups[i]) + ", allowed are 1 .. " + std::to_string(PS_KMER_MAX_GROUPS));
        if (as[i]->E > 0) PS_TRY(stats_output(who, "groups", groups ? groups[i] : nullptr));
        for (int e = 0; e < as[i]->E; e++)
            if (groups[i][e] < 0 || groups[i][e] >= n_groups[i])
                return fail(PS_ERR_BAD_ARG, who + ": event " + std::to_string(e) + " has group " + std::to_string(groups[i][e]) + ", n_groups = " + std::to_string(n_groups[i]));
        PS_TRY(stats_scores(who, realign, scores, i, &rq[i]));
        rq[i].a = as[i]; rq[i].table = table[i]; rq[i].ngroups = n_groups[i]; rq[i].group = groups ? groups[i] : nullptr;
    }
    return stats_run(OwnKind::KmerStats, realign, rq);
}
int ps_kmer_stats(ps_align* a, int32_t realign, const int32_t* groups, int32_t n_groups, double* scores, ps_kmer_cell* table) {
    if (!a) return fail(PS_ERR_BAD_ARG, "ps_kmer_stats: null handle");
    if (!table) return fail(PS_ERR_BAD_ARG, "ps_kmer_stats: null table");
    return ps_batch_kmer_stats(1, &a, realign, &groups, &n_groups, &scores, &table);
}
int ps_batch_move_stats(int32_t n, ps_align* const* a, double* const* scores, ps_event_moves* const* moves, uint8_t* const* const* step,
                        int32_t* const* const* col) {
    const std::string who = "ps_batch_move_stats";
    std::vector<Align*> as;
    PS_TRY(batch_handles(n, a, &as));
    if (n) PS_TRY(stats_output(who, "moves", moves));
    std::vector<OwnReq> rq(n);
    for (int i = 0; i < n; i++) {
        PS_TRY(stats_output(who, "moves", moves[i]));
        PS_TRY(stats_scores(who, 1, scores, i, &rq[i]));
        rq[i].a = as[i]; rq[i].moves = moves[i];
        rq[i].step = step ? step[i] : nullptr; rq[i].col = col ? col[i] : nullptr;
        PS_TRY(stats_levels(who, as[i], (const void* const*)rq[i].step, (const void* const*)rq[i].col));
    }
    return stats_run(OwnKind::MoveStats, 1, rq);
}
int ps_move_stats(ps_align* a, double* scores, ps_event_moves* moves, uint8_t* const* step, int32_t* const* col) {
    if (!a) return fail(PS_ERR_BAD_ARG, "ps_move_stats: null handle");
    if (!moves) return fail(PS_ERR_BAD_ARG, "ps_move_stats: null moves");
    return ps_batch_move_stats(1, &a, &scores, &moves, &step, &col);
}
int ps_batch_posterior_stats(int32_t n, ps_align* const* a, ps_event_posterior* const* stats, double* const* const* emit, double* const* const* col) {
    const std::string who = "ps_batch_posterior_stats";
    std::vector<Align*> as;
    PS_TRY(batch_handles(n, a, &as));
    if (n) PS_TRY(stats_output(who, "stats", stats));
    if ((emit == nullptr) != (col == nullptr)) return fail(PS_ERR_BAD_ARG, who + ": emit and col go together");
    std::vector<OwnReq> rq(n);
    for (int i = 0; i < n; i++) {
        PS_TRY(stats_output(who, "stats", stats[i]));
        if (!as[i]->nonfinite.empty())
            return fail(PS_ERR_BAD_ARG, who + ": " + as[i]->nonfinite + " (the sum over alignments needs finite levels with stdv > 0 and a model with positive deviations)");
        rq[i].a = as[i]; rq[i].post = stats[i];
        rq[i].emit = emit ? emit[i] : nullptr; rq[i].pcol = col ? col[i] : nullptr;
        if ((rq[i].emit == nullptr) != (rq[i].pcol == nullptr)) return fail(PS_ERR_BAD_ARG, who + ": emit and col go together");
        PS_TRY(stats_levels(who, as[i], (const void* const*)rq[i].emit, (const void* const*)rq[i].pcol));
    }
    return stats_run(OwnKind::Posterior, 0, rq);
}
int ps_posterior_stats(ps_align* a, ps_event_posterior* stats, double* const* emit, double* const* col) {
    if (!a) return fail(PS_ERR_BAD_ARG, "ps_posterior_stats: null handle");
    if (!stats) return fail(PS_ERR_BAD_ARG, "ps_posterior_stats: null stats");
    return ps_batch_posterior_stats(1, &a, &stats, emit ? &emit : nullptr, col ? &col : nullptr);
}
int ps_batch_find_mutations(int32_t n, ps_align* const* a, const ps_seqs* const* seeds, ps_muts** out) {
    std::vector<Align*> as;
    PS_TRY(batch_handles(n, a, &as));
    if (n && (!seeds || !out)) return fail(PS_ERR_BAD_ARG, "ps_batch_find_mutations");
    NEED_RT();
    std::vector<std::unique_ptr<ps_muts>> m(n);
    std::vector<const std::vector<std::string>*> sd(n);
    std::vector<std::vector<Mut>*> o(n);
    for (int i = 0; i < n; i++) {
        if (!seeds[i]) return fail(PS_ERR_BAD_ARG, "ps_batch_find_mutations: null seeds");
        m[i].reset(new ps_muts()); sd[i] = &seeds[i]->v; o[i] = &m[i]->v;
    }
    PS_TRY(find_mutations_multi(rt, as, sd, o));
    for (int i = 0; i < n; i++) out[i] = m[i].release();
    return PS_OK;
}
int ps_score_sequences(ps_align* a, int32_t n_seqs, const int64_t* off, const char* pool, double* scores, double* accuracy) {
    if (!a || n_seqs < 0 || (n_seqs && (!off || !pool)) || (n_seqs && a->a.E && !scores)) return fail(PS_ERR_BAD_ARG, "ps_score_sequences");
    if (n_seqs && off[0] < 0) return fail(PS_ERR_BAD_ARG, "ps_score_sequences: negative offset");
    for (int i = 0; i < n_seqs; i++) if (off[i + 1] < off[i]) return fail(PS_ERR_BAD_ARG, "ps_score_sequences: offsets not monotone");
    NEED_RT();
    std::vector<std::string> sv;
    for (int i = 0; i < n_seqs; i++) sv.emplace_back(pool + off[i], pool + off[i + 1]);
    return score_sequences_multi(rt, {&a->a}, {&sv}, {scores}, {accuracy});
}
int ps_batch_score_sequences(int32_t n, ps_align* const* a, const ps_seqs* const* seqs, double* const* scores, double* const* accuracy) {
    std::vector<Align*> as;
    PS_TRY(batch_handles(n, a, &as));
    if (n && (!seqs || !scores)) return fail(PS_ERR_BAD_ARG, "ps_batch_score_sequences");
    NEED_RT();
    std::vector<const std::vector<std::string>*> sv(n);
    std::vector<double*> sc(n), ac(n);
    for (int i = 0; i < n; i++) {
        if (!seqs[i]) return fail(PS_ERR_BAD_ARG, "ps_batch_score_sequences: null sequences");
        if (!scores[i] && as[i]->E && !seqs[i]->v.empty()) return fail(PS_ERR_BAD_ARG, "ps_batch_score_sequences: null scores");
        sv[i] = &seqs[i]->v; sc[i] = scores[i]; ac[i] = accuracy ? accuracy[i] : nullptr;
    }
    return score_sequences_multi(rt, as, sv, sc, ac);
}
int ps_batch_score_mutations(int32_t n, ps_align* const* a, const ps_muts* const* muts, ps_muts** out) {
    std::vector<Align*> as;
    PS_TRY(batch_handles(n, a, &as));
    if (n && (!muts || !out)) return fail(PS_ERR_BAD_ARG, "ps_batch_score_mutations");
    NEED_RT();
    std::vector<std::unique_ptr<ps_muts>> m(n);
    std::vector<EditReq> rq(n);
    for (int i = 0; i < n; i++) {
        if (!muts[i]) return fail(PS_ERR_BAD_ARG, "ps_batch_score_mutations: null list");
        m[i].reset(new ps_muts()); rq[i].a = as[i]; rq[i].muts = &muts[i]->v; rq[i].out = &m[i]->v;
    }
    PS_TRY(score_edits(rt, EditKind::List, rq.data(), rq.size()));
    for (int i = 0; i < n; i++) out[i] = m[i].release();
    return PS_OK;
}
int ps_batch_point_table(int32_t n_regions, ps_align* const* a, double* const* table, ps_point_best* const* best, const int64_t* n) {
    std::vector<Align*> as;
    PS_TRY(batch_handles(n_regions, a, &as));
    if (n_regions && !n) return fail(PS_ERR_BAD_ARG, "ps_batch_point_table: null position counts");
    std::vector<EditReq> rq(n_regions);
    for (int i = 0; i < n_regions; i++) { rq[i].a = as[i]; rq[i].table = table ? table[i] : nullptr; rq[i].best = best ? best[i] : nullptr; rq[i].npos_given = n[i]; }
    // ScorePoints (ScoreMutations on FindPointMutations' list, at the scoring width the AlignData carries), reduced on the device to a
    // row per position (k_point_table) instead of a scored list
    return score_edits(nullptr, EditKind::Points, rq.data(), rq.size());
}
int ps_point_table(ps_align* a, double* table, ps_point_best* best, int64_t n) {
    if (!a) return fail(PS_ERR_BAD_ARG, "ps_point_table: null handle");
    return ps_batch_point_table(1, &a, &table, &best, &n);
}
int ps_batch_score_mutation_support(int32_t n, ps_align* const* a, const ps_muts* const* muts, const int32_t* n_groups,
                                    const int32_t* const* group, double* const* scores, ps_edit_support* const* support) {
    std::vector<Align*> as;
    PS_TRY(batch_handles(n, a, &as));
    if (n && (!muts || !n_groups || !group || !support)) return fail(PS_ERR_BAD_ARG, "ps_batch_score_mutation_support: null array");
    std::vector<EditReq> rq(n);
    for (int i = 0; i < n; i++) {
        EditReq& q = rq[i];
        q.a = as[i]; q.muts = muts[i] ? &muts[i]->v : nullptr; q.group = group[i]; q.ngroups = n_groups[i]; q.score = scores ? scores[i] : nullptr; q.rec = support[i];
    }
    return score_edits(nullptr, EditKind::Support, rq.data(), rq.size());   // k_support instead of k_reduce behind k_score
}
int ps_score_mutation_support(ps_align* a, const ps_muts* muts, int32_t n_groups, const int32_t* group, double* scores, ps_edit_support* support) {
    if (!a) return fail(PS_ERR_BAD_ARG, "ps_score_mutation_support: null handle");
    return ps_batch_score_mutation_support(1, &a, &muts, &n_groups, &group, &scores, &support);
}
int ps_batch_score_mutation_genotypes(int32_t n, ps_align* const* a, const ps_muts* const* muts, const int32_t* n_groups,
                                      const int32_t* const* group, const int32_t* n_frac, const double* const* alt_frac,
                                      double* const* scores, ps_edit_support* const* support, double* const* lik, int32_t* const* n_cover) {
    std::vector<Align*> as;
    PS_TRY(batch_handles(n, a, &as));
    if (n && (!muts || !n_groups || !group || !n_frac || !lik)) return fail(PS_ERR_BAD_ARG, "ps_batch_score_mutation_genotypes: null array");
    std::vector<EditReq> rq(n);
    for (int i = 0; i < n; i++) {
        EditReq& q = rq[i];
        q.a = as[i]; q.muts = muts[i] ? &muts[i]->v : nullptr; q.group = group[i]; q.ngroups = n_groups[i]; q.nfrac = n_frac[i]; q.frac = alt_frac ? alt_frac[i] : nullptr;
        q.score = scores ? scores[i] : nullptr; q.rec = support ? support[i] : nullptr; q.lik = lik[i]; q.ncover = n_cover ? n_cover[i] : nullptr;
    }
    return score_edits(nullptr, EditKind::Genotype, rq.data(), rq.size());   // k_genotype behind k_support
}
int ps_score_mutation_genotypes(ps_align* a, const ps_muts* muts, int32_t n_groups, const int32_t* group, int32_t n_frac, const double* alt_frac,
                                double* scores, ps_edit_support* support, double* lik, int32_t* n_cover) {
    if (!a) return fail(PS_ERR_BAD_ARG, "ps_score_mutation_genotypes: null handle");
    return ps_batch_score_mutation_genotypes(1, &a, &muts, &n_groups, &group, &n_frac, &alt_frac, &scores, &support, &lik, &n_cover);
}
int ps_batch_score_mutation_phase(int32_t n, ps_align* const* a, const ps_muts* const* muts, const int32_t* window, const double* min_link,
                                  const int32_t* max_sets, double* const* scores, ps_edit_link* const* link, ps_edit_phase* const* phase,
                                  ps_event_hap* const* hap, int32_t* const* n_sets) {
    std::vector<Align*> as;
    PS_TRY(batch_handles(n, a, &as));
    if (n && (!muts || !window || !min_link || !max_sets || !link || !phase)) return fail(PS_ERR_BAD_ARG, "ps_batch_score_mutation_phase: null array");
    std::vector<EditReq> rq(n);
    for (int i = 0; i < n; i++) {
        EditReq& q = rq[i];
        q.a = as[i]; q.muts = muts[i] ? &muts[i]->v : nullptr; q.window = window[i]; q.min_link = min_link[i]; q.max_sets = max_sets[i];
        q.score = scores ? scores[i] : nullptr; q.link = link[i]; q.phase = phase[i];
        q.hap = hap ? hap[i] : nullptr; q.nsets = n_sets ? n_sets[i] : nullptr;
    }
    return score_edits(nullptr, EditKind::Phase, rq.data(), rq.size());   // k_link, k_phase and k_haptag behind k_score
}
int ps_score_mutation_phase(ps_align* a, const ps_muts* muts, int32_t window, double min_link, int32_t max_sets, double* scores,
                            ps_edit_link* link, ps_edit_phase* phase, ps_event_hap* hap, int32_t* n_sets) {
    if (!a) return fail(PS_ERR_BAD_ARG, "ps_score_mutation_phase: null handle");
    return ps_batch_score_mutation_phase(1, &a, &muts, &window, &min_link, &max_sets, &scores, &link, &phase, &hap, &n_sets);
}
int ps_batch_make_mutations(int32_t n, ps_align* const* a, const ps_muts* const* scored, int32_t* n_bases) {
    std::vector<Align*> as;
    PS_TRY(batch_handles(n, a, &as));
    if (n && (!scored || !n_bases)) return fail(PS_ERR_BAD_ARG, "ps_batch_make_mutations");
    NEED_RT();
    std::vector<std::vector<Mut>> in(n);
    for (int i = 0; i < n; i++) if (!scored[i]) return fail(PS_ERR_BAD_ARG, "ps_batch_make_mutations: null list");
    par_for(n, [&](int i) { in[i] = scored[i]->v; });   // (a Refine list is 80 000 edits per region: the copies run side by side)
    std::vector<int> nb;
    PS_TRY(make_mutations_multi(rt, as, std::move(in), &nb));
    for (int i = 0; i < n; i++) n_bases[i] = nb[i];
    return PS_OK;
}
int ps_batch_viterbi_mutate(int32_t n, ps_align* const* a, ps_rng* const* rng, int32_t nkeep, double skip, double stay,
                            double mmin, double mmax, ps_seqs** out) {
    std::vector<Align*> as;
    PS_TRY(batch_handles(n, a, &as));
    if (n && !out) return fail(PS_ERR_BAD_ARG, "ps_batch_viterbi_mutate");
    std::vector<std::unique_ptr<ps_seqs>> s(n);
    std::vector<VitReq> rq(n);
    for (int i = 0; i < n; i++) { s[i].reset(new ps_seqs()); rq[i].a = as[i]; rq[i].rng = (rng && rng[i]) ? rng[i]->s : nullptr; rq[i].out = &s[i]->v; }
    VitCall call;
    call.nkeep = nkeep; call.skip = skip; call.stay = stay; call.mmin = mmin; call.mmax = mmax;
    PS_TRY(viterbi_mutate(nullptr, call, rq.data(), rq.size()));
    for (int i = 0; i < n; i++) out[i] = s[i].release();
    return PS_OK;
}

int ps_swfull(const char* s1, int64_t n1, const char* s2, int64_t n2, int32_t* score, double* acc,
              int32_t* i1, int32_t* i2, int64_t cap, int64_t* np) {
    if (!s1 || !s2 || n1 < 0 || n2 < 0 || !np) return fail(PS_ERR_BAD_ARG, "ps_swfull");
    NEED_RT();
    int sc = 0; double ac = 0;
    std::vector<int> a, b;
    PS_TRY(sw_device(rt, std::string(s1, n1), std::string(s2, n2), &sc, &ac, &a, &b));
    if ((int64_t)a.size() > cap) return fail(PS_ERR_BAD_ARG, "ps_swfull: index capacity too small");
    if (score) *score = sc;
    if (acc) *acc = ac;
    for (size_t k = 0; k < a.size(); k++) { if (i1) i1[k] = a[k]; if (i2) i2[k] = b[k]; }
    *np = (int64_t)a.size();
    return PS_OK;
}
int ps_batch_sw_summary(int64_t n, const char* const* seq1, const int64_t* n1, const char* const* seq2, const int64_t* n2,
                        ps_sw_summary* out) {
    if (n < 0 || (n && (!seq1 || !n1 || !seq2 || !n2 || !out))) return fail(PS_ERR_BAD_ARG, "ps_batch_sw_summary");
    for (int64_t k = 0; k < n; k++)
        if (n1[k] < 0 || n2[k] < 0 || (n1[k] && !seq1[k]) || (n2[k] && !seq2[k])) return fail(PS_ERR_BAD_ARG, "ps_batch_sw_summary: bad pair");
    if (!n) return PS_OK;
    NEED_RT();
    std::vector<std::string> s(2 * (size_t)n);
    SwInput in;
    for (int64_t k = 0; k < n; k++) {
        if (n1[k]) s[2 * k].assign(seq1[k], (size_t)n1[k]);
        if (n2[k]) s[2 * k + 1].assign(seq2[k], (size_t)n2[k]);
    }
    for (int64_t k = 0; k < n; k++) in.push_back({&s[2 * k], &s[2 * k + 1]});
    std::vector<SwResult> res;
    PS_TRY(sw_summaries(rt, in, &res));
    for (int64_t k = 0; k < n; k++) {
        const SwResult& r = res[k];
        ps_sw_summary& o = out[k];
        o.score = r.score; o.n_pairs = r.n_pairs; o.n_match = r.n_match;
        o.first1 = r.first1; o.first2 = r.first2; o.last1 = r.last1; o.last2 = r.last2;
        o.gap1 = r.gap1; o.gap2 = r.gap2;
        o.accuracy = r.accuracy;
    }
    return PS_OK;
}
int ps_seq_to_states(const char* seq, int64_t n, int32_t* st, int64_t* ns) {
    if (!seq || n < 0 || !ns) return fail(PS_ERR_BAD_ARG, "ps_seq_to_states");
    std::vector<int> v = states_of(std::string(seq, n));  // pure index arithmetic, no DP: host
    if (st) std::copy(v.begin(), v.end(), st);
    *ns = (int64_t)v.size();
    return PS_OK;
}

// Smith-Waterman band mode counters (process-wide, cumulative; a test hook outside the public header): out[0] pairs run in band mode,
// out[1] of them redone on the full matrix after a failed certificate, out[2] certified pairs whose maximum lies within 64 of the band
// edge, out[3] cells the fills computed, out[4] full-matrix cells of the same pairs
int ps_debug_sw_band(int64_t* out) {
    if (!out) return fail(PS_ERR_BAD_ARG, "ps_debug_sw_band");
    sw_band_counters(out);
    return PS_OK;
}
int ps_debug_posterior(ps_align* a, int32_t e, double* main, double* stay) {
    if (!a || e < 0 || e >= a->a.E || !main) return fail(PS_ERR_BAD_ARG, "ps_debug_posterior");
    if (!a->a.nonfinite.empty()) return fail(PS_ERR_BAD_ARG, "ps_debug_posterior: " + a->a.nonfinite);
    NEED_RT();
    return debug_posterior(rt, &a->a, e, main, stay);
}
int ps_debug_fill(ps_align* a, int32_t e, int32_t dir, double* main, double* stay, uint8_t* sm, uint8_t* ss) {
    if (!a || e < 0 || e >= a->a.E || !main || dir < 0 || dir > 1) return fail(PS_ERR_BAD_ARG, "ps_debug_fill");
    NEED_RT();
    return debug_fill(rt, &a->a, e, dir, main, stay, sm, ss);
}
int ps_debug_poison(uint32_t index_word, uint64_t value_word, ps_poison_report* report, int32_t cap, int32_t* n_report) {
    if (cap < 0 || (cap && !report)) return fail(PS_ERR_BAD_ARG, "ps_debug_poison");
    NEED_RT();
    return debug_poison(rt, index_word, value_word, report, cap, n_report);
}
int ps_debug_viterbi(int32_t n, ps_align* const* a, int32_t build, int32_t nkeep, double skip, double stay, double mmin, double mmax,
                     int64_t cap_T, int32_t* T, double* obs, int16_t* bp, double* lik_final, double* fwd, int16_t* paths) {
    std::vector<Align*> as;
    PS_TRY(batch_handles(n, a, &as));
    if (nkeep < 0 || build < 0 || build > 3 || cap_T < 0 || (n && !T)) return fail(PS_ERR_BAD_ARG, "ps_debug_viterbi");
    return debug_viterbi(as, build, nkeep, skip, stay, mmin, mmax, cap_T, T, obs, bp, lik_final, fwd, paths);
}
int ps_debug_viterbi_steps(int32_t R, const int32_t* T, const double* obs, const double* rnd, int32_t nkeep, double skip, double stay,
                           double mmin, double mmax, int16_t* bp, double* lik_final, double* fwd, int16_t* paths) {
    if (R < 0 || nkeep < 0 || (R && !T)) return fail(PS_ERR_BAD_ARG, "ps_debug_viterbi_steps");
    int64_t ttot = 0;
    for (int r = 0; r < R; r++) { if (T[r] < 0) return fail(PS_ERR_BAD_ARG, "ps_debug_viterbi_steps: negative T"); ttot += T[r]; }
    if (ttot && (!obs || (nkeep && !rnd))) return fail(PS_ERR_BAD_ARG, "ps_debug_viterbi_steps: null rows or deviates");
    NEED_RT();
    return debug_viterbi_steps(rt, R, T, obs, rnd, nkeep, skip, stay, mmin, mmax, bp, lik_final, fwd, paths);
}

int ps_srand(uint32_t seed) { rand_seed(seed); return PS_OK; }
int ps_rand_draw(int64_t n, double* out) {
    if (n < 0 || (n && !out)) return fail(PS_ERR_BAD_ARG, "ps_rand_draw");
    for (int64_t k = 0; k < n; k++) out[k] = rand_next() / (double(RAND_MAX) + 1);
    return PS_OK;
}

int ps_set_sweep_min(int32_t n) { sweep_min_set(n); return PS_OK; }
int ps_set_sweep2_min(int32_t n) { sweep2_min_set(n); return PS_OK; }
int ps_set_sparse_min(int32_t n) { sparse_min_set(n); return PS_OK; }
int ps_set_device_fraction(double f) {
    if (f > 1.0) return fail(PS_ERR_BAD_ARG, "ps_set_device_fraction: a fraction in (0, 1]; <= 0 restores the default");
    device_fraction_set(f);
    return PS_OK;
}
int ps_set_sweep_form(int32_t K, int32_t NW) {
    if (K <= 0 && NW > 0 && NW != 1 && NW != 2 && NW != 4) return fail(PS_ERR_BAD_ARG, "ps_set_sweep_form: 1, 2 or 4 wavefronts per sweep");
    if (K > 0 && !sweep_form_exists(K, NW)) return fail(PS_ERR_BAD_ARG, "ps_set_sweep_form: no such form (rows per lane, wavefronts)");
    sweep_form_set(K, NW);
    return PS_OK;
}

int ps_prof_enable(int32_t on) {
    NEED_RT();
    prof_flush(rt);
    rt->prof_on = on != 0;
    rt->prof_defer = on == 2;
    return PS_OK;
}
int ps_prof_reset(void) {
    NEED_RT();
    prof_flush(rt);
    rt->prof.clear();
    return PS_OK;
}
int ps_prof_get(const char* name, double* ms, int64_t* n, double* bytes) {
    NEED_RT();
    prof_flush(rt);
    Prof p;
    if (name) { auto it = rt->prof.find(name); if (it != rt->prof.end()) p = it->second; }
    if (ms) *ms = p.ms;
    if (n) *n = p.launches;
    if (bytes) *bytes = p.bytes;
    return PS_OK;
}

int ps_prof_units(const char* name, double* units) {
    NEED_RT();
    prof_flush(rt);
    Prof p;
    if (name) { auto it = rt->prof.find(name); if (it != rt->prof.end()) p = it->second; }
    if (units) *units = p.units;
    return PS_OK;
}

}  // extern "C"
