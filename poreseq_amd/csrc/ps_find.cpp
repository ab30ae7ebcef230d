// ps_find.cpp — FindMutations (cpp/FindMutations.cpp:24-186), MapAlignments (cpp/EventUtil.cpp:12-55),
// fillinds (cpp/swlib.cpp:342-365) and the host part of ViterbiMutate (cpp/Viterbi.cpp:239-426).
// The alignments, Smith-Waterman matrices and the Viterbi recursion run on the GPU; what is left
// here is the reference's list / index bookkeeping.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <thread>

#include "ps_extract.h"   // the tail of FindMutations on plain host data (no HIP)
#include "ps_host.h"
#include "ps_sw.h"

namespace ps {

// PORESEQ_DEBUG_LIKES_HOST=1 (tests; read per call): every chunk's per-base likelihood vectors come from the host loop
static bool likes_on_host() { const char* e = getenv("PORESEQ_DEBUG_LIKES_HOST"); return e && atoi(e) != 0; }

static void fillinds(SwResult& al) {  // cpp/swlib.cpp:342-365
    if (al.a.empty()) return;
    int i1 = al.a[0], i2 = al.b[0];
    for (size_t k = 0; k < al.a.size(); k++) {
        if (al.a[k] > 0) i1 = al.a[k]; else al.a[k] = i1;
        if (al.b[k] > 0) i2 = al.b[k]; else al.b[k] = i2;
    }
}

namespace {
// FindMutations (cpp/FindMutations.cpp:24-186) for several AlignData in lock-step: one Smith-Waterman batch for all
// (sequence, seed) pairs, one base realign over all events, the candidate-sequence alignments of all regions in as few
// launch chains as device memory allows, then the host-side extraction per AlignData on host threads.
// One call on its way through the stages below, which fill it in this order
struct Find {
    Runtime* rt;
    const std::vector<Align*>& as;
    const std::vector<const std::vector<std::string>*>& seeds;
    int R;
    Tick tk;
    SwInput pairs;                 // (current sequence, seed) of every region, region by region; region r's from pair0[r] on
    std::vector<int> pair0, wbs;   // wbs: the band half-width of every pair
    SwJob swjob;                   // the first Smith-Waterman launch, in flight on the second stream
    size_t sw_first = 0;           // pairs in it
    std::vector<SwResult> als;     // per pair
    std::vector<std::vector<double>> base;   // per region: the per-base cumulative likelihoods of its current sequence
    struct Need { int r, k; std::vector<int> states; };
    std::vector<Need> need;        // (region, seed) pairs whose likelihood vector is not cached yet
    Find(Runtime* rt_, const std::vector<Align*>& as_, const std::vector<const std::vector<std::string>*>& seeds_)
        : rt(rt_), as(as_), seeds(seeds_), R((int)as_.size()), tk("find_mutations") {}
    const std::string& seed(const Need& nd) const { return (*seeds[nd.r])[nd.k]; }
    const SwResult& al(const Need& nd) const { return als[pair0[nd.r] + nd.k]; }
};
}  // namespace

// ---- stage: pairs.  Every current sequence against each of its seeds (MapAlignments, cpp/EventUtil.cpp:16).  Pairs whose alignment
// hugs the main diagonal (the Viterbi seeds) run in band mode (ps_sw.hip), with checkpoints sized from the band.
static void pair_up(Find& f) {
    f.pair0.assign(f.R + 1, 0);
    for (int r = 0; r < f.R; r++) {
        f.pair0[r] = (int)f.pairs.size();
        for (const std::string& s : *f.seeds[r]) f.pairs.push_back({&f.as[r]->bases, &s});
    }
    f.pair0[f.R] = (int)f.pairs.size();
    f.wbs.resize(f.pairs.size());
    for (size_t k = 0; k < f.pairs.size(); k++) f.wbs[k] = sw_band_choice(*f.pairs[k].first, *f.pairs[k].second);
}

// ---- stage: first Smith-Waterman launch.  Independent of the re-alignment below, so it runs concurrently on the second stream.
// The batch's checkpoint rows / columns (~13 MB per 10 kb pair) are a pool like the DP matrices: at most an eighth of this
// runtime's share goes into one launch.  The first chunk overlaps with the base realign; what is left (large lock-step batches
// only) follows it, chunk by chunk, and a chunk the device has no memory for is cut in two (sw_drain).
static int sw_enqueue(Find& f) {
    f.sw_first = sw_chunk_end(f.pairs, f.wbs.data(), SW_LISTS, 0, sw_chunk_cap());
    const int rc = sw_launch(f.rt, SwInput(f.pairs.begin(), f.pairs.begin() + f.sw_first), &f.swjob, f.wbs.data());
    if (rc == PS_ERR_NOMEM && f.sw_first > 1) { f.sw_first = 0; f.swjob = SwJob(); }   // nothing enqueued: everything goes the chunked way below
    else PS_TRY(rc);
    f.tk.lap("sw enqueue");
    return PS_OK;
}

// ---- stage: base realign.  Re-align to the current sequences, keeping per-base cumulative likelihoods (cpp/FindMutations.cpp:28-29).
// Its error is the caller's to return once the second stream has been drained.
static int base_realign(Find& f) {
    std::vector<std::vector<double>> sc(f.R);
    std::vector<OwnReq> rq(f.R);
    f.base.resize(f.R);
    for (int r = 0; r < f.R; r++) {
        f.base[r].assign(std::max<size_t>(f.as[r]->bases.size(), 4) + 1, 0.0);
        sc[r].assign(std::max(f.as[r]->E, 1), 0.0);
        rq[r].a = f.as[r]; rq[r].scores = sc[r].data(); rq[r].likes = f.base[r].data();
    }
    const int rc = own_forward(f.rt, OwnKind::Score, true, rq.data(), rq.size());
    f.tk.lap("base realign");
    return rc;
}

// ---- stage: drain, and the Smith-Waterman chunks that did not go with the realign
static int sw_drain(Find& f, int rc_base) {
    PS_TRY(sw_finish(f.rt, &f.swjob, &f.als));   // always drain the second stream, even on failure above
    PS_TRY(rc_base);
    PS_TRY(sw_chunks(f.rt, f.pairs, f.wbs.data(), SW_LISTS, f.sw_first, &f.als));
    if (f.sw_first < f.pairs.size()) { if (trace_on()) fprintf(stderr, "[ps] smith-waterman: %zu pairs, %zu with the realign, the rest in chunks\n", f.pairs.size(), f.sw_first); }
    return PS_OK;
}

// ---- stage: fillinds (cpp/swlib.cpp:342-365) of every pair's lists
static void fill_indices(Find& f) {
    // the reference's progress line under `verbose` (cpp/FindMutations.cpp:34-35, 100-109: "Finding mutations", a dot per seed sequence, a
    // newline); single-handle calls only (a lock-step call has no single line to write)
    if (f.R == 1 && f.as[0]->par.verbose) {
        fputs("Finding mutations", stderr);
        for (size_t k = 0; k < f.seeds[0]->size(); k++) fputc('.', stderr);
        fputc('\n', stderr);
        fflush(stderr);
    }
    par_for((int)f.als.size(), [&](int k) { fillinds(f.als[k]); });
    f.tk.lap("smith-waterman");
}

// ---- stage: needs.  (region, seed) pairs whose likelihood vector is not in the AlignData's cache (seqlikes, cpp/AlignData.h:34) get
// (seed x event) alignment jobs; a repeated seed once; without events the vector is zeros
static void list_needs(Find& f) {
    for (int r = 0; r < f.R; r++) {
        Align* a = f.as[r];
        const std::vector<std::string>& sd = *f.seeds[r];
        std::map<std::string, int> seen;
        for (int k = 0; k < (int)sd.size(); k++) {
            if (!a->seqlikes[sd[k]].empty()) continue;
            if (seen.count(sd[k])) continue;
            seen[sd[k]] = k;
            if (a->E) f.need.push_back({r, k, {}});
            else a->seqlikes[sd[k]] = std::vector<double>(sd[k].size(), 0.0);
        }
    }
}

// ---- stage: seed likelihoods, through fwd_chunks (ps_fwd.cpp).
// place: the remapped ref_align of every (seed, event) job of the chunk (cpp/EventUtil.cpp:22-51; map_alignment, ps_extract.h), made
// on the host into pinned memory and enqueued
static int place_seed_refs(Find& f, FwdChunk& c) {
    double* h_ra = (double*)f.rt->stage.alloc(std::max<size_t>(c.nref, 1) * sizeof(double));   // pinned: plain enqueue below
    if (!h_ra) return fail(PS_ERR_NOMEM, "hipHostMalloc (staging arena)");
    par_for((int)(c.q1 - c.q0), [&](int qq) {
        const Find::Need& nd = f.need[c.q0 + qq];
        const Align* a = f.as[nd.r];
        const SwResult& al = f.al(nd);
        double* dst = h_ra + c.roff[qq];
        for (int64_t t = 0; t < a->ntot; t++) dst[t] = map_alignment(al.a, al.b, (int)a->h_ra[t]);
    });
    f.tk.lap("remap (host)");
    if (c.nref) PS_HIP(hipMemcpyAsync(c.d_ra, h_ra, c.nref * sizeof(double), hipMemcpyHostToDevice, f.rt->stream));
    PS_HIP(hipMemsetAsync(c.d_rl, 0, std::max<size_t>(c.nref, 1) * sizeof(double), f.rt->stream));
    return PS_OK;
}

// collect: the per-base likelihood vectors of the chunk's sequences, into the AlignData's caches: on the device when every sequence
// fits k_likes' table (only the vectors cross PCIe), else from the jobs' ref_align / ref_like on the host
static int collect_likes(Find& f, FwdChunk& c) {
    Runtime* rt = f.rt;
    const size_t n = c.q1 - c.q0;
    std::vector<std::vector<double>> lks(n);
    bool on_device = true;
    for (size_t q = c.q0; q < c.q1; q++) if ((int)f.need[q].states.size() > likes_max_states()) on_device = false;
    if (likes_on_host()) on_device = false;
    if (rt->prof_on) rt->prof[on_device ? "likes_dev" : "likes_host"].launches++;   // (chunks that took each path: host-side counts)
    if (on_device) {
        std::vector<LikeGroup> groups(n);
        int64_t out_tot = 0;
        int job = 0;
        for (size_t qq = 0; qq < n; qq++) {
            const Find::Need& nd = f.need[c.q0 + qq];
            LikeGroup& g = groups[qq];
            g.job0 = job; g.njobs = f.as[nd.r]->E; job += g.njobs;
            g.C = (int)nd.states.size(); g.len = (int)f.seed(nd).size();
            g.out_off = out_tot; out_tot += g.len;
        }
        DBuf& gb = rt->buf("like_groups");
        DBuf& lb = rt->buf("like_out");
        PS_TRY(gb.ensure(groups.size() * sizeof(LikeGroup)));
        PS_TRY(lb.ensure((size_t)std::max<int64_t>(out_tot, 1) * sizeof(double)));
        PS_TRY(rt->up(gb.p, groups.data(), groups.size() * sizeof(LikeGroup)));
        PS_TRY(launch_likes(rt, c.b.d, gb.as<LikeGroup>(), (int)groups.size(), lb.as<double>()));
        double* h_lk = nullptr;
        PS_TRY(rt->down(&h_lk, lb.p, (size_t)out_tot));
        PS_HIP(hipStreamSynchronize(rt->stream));
        f.tk.lap("seed realign + D2H");
        for (size_t qq = 0; qq < n; qq++) lks[qq].assign(h_lk + groups[qq].out_off, h_lk + groups[qq].out_off + groups[qq].len);
    } else {
        double *r_ra = nullptr, *r_rl = nullptr;
        PS_TRY(rt->down(&r_ra, c.d_ra, c.nref));
        PS_TRY(rt->down(&r_rl, c.d_rl, c.nref));
        PS_HIP(hipStreamSynchronize(rt->stream));
        f.tk.lap("seed realign + D2H");
        par_for((int)n, [&](int qq) {
            const Find::Need& nd = f.need[c.q0 + qq];
            const Align* a = f.as[nd.r];
            const std::string& sd = f.seed(nd);
            std::vector<double>& lk = lks[qq];
            lk.assign(std::max<size_t>(sd.size(), 4) + 1, 0.0);
            for (int e = 0; e < a->E; e++) {
                const size_t o = c.roff[qq] + a->off[e];
                accumulate_likes(r_ra + o, r_rl + o, a->n[e], (int)nd.states.size(), lk.data());
            }
            lk.resize(sd.size());
        });
    }
    for (size_t qq = 0; qq < n; qq++) { const Find::Need& nd = f.need[c.q0 + qq]; f.as[nd.r]->seqlikes[f.seed(nd)] = std::move(lks[qq]); }
    return PS_OK;
}

static int seed_likes(Find& f) {
    {   // host mirrors of ref_align for the remap: one synchronisation for all
        for (int r = 0; r < f.R; r++) PS_TRY(f.as[r]->refs_to_host_async(f.rt));
        PS_HIP(hipStreamSynchronize(f.rt->stream));
        for (int r = 0; r < f.R; r++) f.as[r]->refs_finish();
    }
    par_for((int)f.need.size(), [&](int q) { f.need[q].states = states_of(f.seed(f.need[q])); });
    std::vector<FwdUnit> units(f.need.size());
    for (size_t q = 0; q < f.need.size(); q++) units[q] = {f.as[f.need[q].r], &f.need[q].states};
    return fwd_chunks(f.rt, units, "seed", [&](FwdChunk& c) { return place_seed_refs(f, c); }, [&](FwdChunk& c) { return collect_likes(f, c); }, nullptr, &f.tk);
}

// ---- stage: extraction.  Likelihood differences -> clamped CUSUM -> greedy extraction (ps_extract.h), per AlignData
static int extract(Find& f, const std::vector<std::vector<Mut>*>& outs) {
    std::vector<int> rcs(f.R, PS_OK);
    par_for(f.R, [&](int r) {
        const std::vector<std::string>& sd = *f.seeds[r];
        std::vector<std::vector<int>> ia(sd.size()), ib(sd.size());
        std::vector<const std::vector<double>*> lk(sd.size());
        for (size_t k = 0; k < sd.size(); k++) {
            ia[k] = std::move(f.als[f.pair0[r] + k].a); ib[k] = std::move(f.als[f.pair0[r] + k].b);
            lk[k] = &f.as[r]->seqlikes[sd[k]];
        }
        if (extract_edits(f.as[r]->bases, sd, ia, ib, f.base[r], lk, outs[r])) rcs[r] = PS_ERR_BAD_ARG;
    });
    for (int r = 0; r < f.R; r++) if (rcs[r] != PS_OK) return fail(rcs[r], "FindMutations: alignment index outside the sequence");
    f.tk.lap("extract");
    return PS_OK;
}

int find_mutations_multi(Runtime* rt, const std::vector<Align*>& as, const std::vector<const std::vector<std::string>*>& seeds,
                         const std::vector<std::vector<Mut>*>& outs) {
    Find f(rt, as, seeds);
    for (int r = 0; r < f.R; r++) outs[r]->clear();
    pair_up(f);
    PS_TRY(sw_enqueue(f));
    const int rc_base = base_realign(f);
    PS_TRY(sw_drain(f, rc_base));
    if (f.pairs.empty()) return PS_OK;
    fill_indices(f);
    list_needs(f);
    if (!f.need.empty()) PS_TRY(seed_likes(f));
    f.tk.lap("seed likes");
    return extract(f, outs);
}

int find_mutations(Runtime* rt, Align* a, const std::vector<std::string>& seeds, std::vector<Mut>* out) {
    return find_mutations_multi(rt, {a}, {&seeds}, {out});
}

// ---------------------------------------------------------------------------------------------
inline int succ(int st, int k, int j) { return ((st << (2 * j)) & (NS - 1)) + k; }   // cpp/Viterbi.h:31-32
inline char base_at(int st, int k) { return "ACGT"[3 & (st >> (2 * (4 - k)))]; }    // cpp/Viterbi.h:35-39

// StatesToSequence, cpp/Viterbi.cpp:171-237
static std::string path_to_bases(const std::vector<int>& st) {
    std::string s;
    int cur = st[0];
    s.push_back(base_at(cur, 0));
    for (size_t i = 1; i < st.size(); i++) {
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

namespace {
// host part of ViterbiMutate for one AlignData: which reference positions are kept and the mean level per (position, event)
struct VitGather { std::vector<double> obsin; int T = 0; };
}  // namespace

// The walk runs from the smallest refstart to the largest refend, both (int)ref_align of an aligned level (cpp/EventData.h:135-136):
// an entry that is not below 2^31, +inf included, has no defined conversion and would send vit_gather towards 2^31 — refused, naming
// the event and the level (region < 0: not a lock-step call).  The DP and the census take any double (include/poreseq_hip.h).
static int vit_refuses_refs(const Align& a, const char* who, int region) {
    for (int e = 0; e < a.E; e++) {
        const double* ra = a.h_ra.data() + a.off[e];
        for (int t = 0; t < a.n[e]; t++)
            if (ra[t] >= 2147483648.0) {
                char val[64];
                snprintf(val, sizeof(val), "%g", ra[t]);
                return fail(PS_ERR_BAD_ARG, std::string(who) + ": " + (region >= 0 ? "region " + std::to_string(region) + ": " : std::string()) + "event " + std::to_string(e) +
                                                ", level " + std::to_string(t) + ": ref_align = " + val + " is not below 2^31 (ViterbiMutate walks the positions from (int)ref_align)");
            }
    }
    return PS_OK;
}

static void vit_gather(const Align* a, const double* h_ri, const JobOut* info, VitGather* g) {
    const int E = a->E;
    // first level whose ref_index equals an integer position (std::find in getrefstates, cpp/EventData.h:192),
    // as a flat table per event indexed by position + 1 (positions outside [-1, maxpos] never match)
    // (extrapolated ref_index values past refend can be integers too and do take part, so the table
    // spans every integer-valued entry).  The table starts at position -1: a read without an aligned level has refstart = -1, the
    // walk then begins there, and std::find meets the -1 markers that an un-interpolated hole keeps (behind an aligned level 0,
    // cpp/EventData.h:157) or a head that the line through the end levels crosses at -1; no position lies below -1.
    int maxpos = 0;
    for (int e = 0; e < E; e++) {
        if (!info[e].has_index) continue;
        const double* ri = h_ri + a->off[e];
        for (int t = 0; t < a->n[e]; t++) {
            const double v = ri[t];
            if (v >= 0.0 && v < 1e9 && v == std::floor(v)) maxpos = std::max(maxpos, (int)v);
        }
    }
    std::vector<std::vector<int>> first(E);
    for (int e = 0; e < E; e++) {
        if (!info[e].has_index) continue;  // empty ref_index: getrefstates finds nothing
        first[e].assign((size_t)maxpos + 2, -1);
        const double* ri = h_ri + a->off[e];
        for (int t = 0; t < a->n[e]; t++) {
            const double v = ri[t];
            if (v >= -1.0 && v <= (double)maxpos && v == std::floor(v)) {
                int& slot = first[e][(size_t)((int)v + 1)];
                if (slot < 0) slot = t;
            }
        }
    }
    auto rstart = [&](int e) { return info[e].has_index ? info[e].refstart : -1; };
    auto rend = [&](int e) { return info[e].has_index ? info[e].refend : -1; };
    int refind = rstart(0);
    for (int e = 0; e < E; e++) refind = std::min(refind, rstart(e));
    std::vector<double>& obsin = g->obsin;
    int T = 0;
    while (true) {
        int nl = 0, nal = 0;
        const size_t at = obsin.size();
        obsin.resize(at + (size_t)E * 4, 0.0);
        for (int e = 0; e < E; e++) {
            if (refind < -1 || refind > maxpos || first[e].empty() || first[e][refind + 1] < 0) continue;
            const double* ra = a->h_ra.data() + a->off[e];
            const double* mean = a->h_mean.data() + a->off[e];
            const double* stdv = a->h_stdv.data() + a->off[e];
            int t = first[e][refind + 1], cnt = 1;
            // getrefstates keeps following levels while ref_align <= refind, using those > 0 (cpp/EventData.h:197-201)
            double lsum = 0, ssum = 0;
            lsum += mean[t]; ssum += stdv[t];
            for (t++; t < a->n[e] && ra[t] <= refind; t++)
                if (ra[t] > 0) { lsum += mean[t]; ssum += stdv[t]; cnt++; }
            const double lvl = lsum / cnt, sd = ssum / cnt;
            nl++;
            double* o = obsin.data() + at + (size_t)e * 4;
            o[0] = lvl; o[1] = sd; o[2] = std::log(sd); o[3] = 1.0;
        }
        for (int e = 0; e < E; e++) if (refind >= rstart(e) && refind <= rend(e)) nal++;
        if (nl <= nal * 0.2) {
            obsin.resize(at);
            if (nal == 0) break;
            refind++;
            continue;
        }
        T++;
        refind++;
    }
    g->T = T;
}

// uniform deviates in the reference's call order: for each kept path, one per back-step (cpp/Viterbi.cpp:108)
static void vit_draw(void* rng, double* rnd, size_t n) {
    RandState* r = (RandState*)rng;
    for (size_t k = 0; k < n; k++) rnd[k] = rand_state_next(r) / (double(RAND_MAX) + 1);
}

// ViterbiMutate (cpp/Viterbi.cpp:239-426) for several AlignData in lock-step; rngs[r] = the region's generator (nullptr: the
// calling thread's); tap: the device tables for ps_debug_viterbi (ps_internal.h), a null pointer otherwise
int viterbi_mutate_multi(Runtime* rt, const std::vector<Align*>& as, const std::vector<RandState*>& rngs, int nkeep, double skip, double stay,
                         double mmin, double mmax, const std::vector<std::vector<std::string>*>& outs, VitTap* tap, const char* who, bool lockstep) {
    Tick tk("viterbi_mutate");
    const int R = (int)as.size();
    for (int r = 0; r < R; r++) outs[r]->clear();
    // host mirrors of ref_align / ref_index / refstart / refend
    std::vector<double*> h_ri(R, nullptr);
    std::vector<JobOut*> info(R, nullptr);
    for (int r = 0; r < R; r++) {
        PS_TRY(as[r]->refs_to_host_async(rt));
        as[r]->last_stream = (void*)rt->stream;
        PS_TRY(rt->down(&h_ri[r], as[r]->d_ri, (size_t)as[r]->ntot));
        PS_TRY(rt->down(&info[r], as[r]->d_out, (size_t)as[r]->E));
    }
    PS_HIP(hipStreamSynchronize(rt->stream));
    for (int r = 0; r < R; r++) as[r]->refs_finish();
    tk.lap("refs D2H");
    for (int r = 0; r < R; r++) PS_TRY(vit_refuses_refs(*as[r], who, lockstep ? r : -1));   // on the host copy, before any kernel of the call
    std::vector<VitGather> gath(R);
    par_for(R, [&](int r) { vit_gather(as[r], h_ri[r], info[r], &gath[r]); });
    tk.lap("gather levels");
    std::vector<VitRegionH> regs(R);
    for (int r = 0; r < R; r++) {
        regs[r].E = as[r]->E; regs[r].T = gath[r].T; regs[r].obsin = gath[r].obsin.data(); regs[r].d_model = as[r]->d_model;
        as[r]->last_stream = (void*)rt->stream;   // (the Viterbi kernels read the model tables in the AlignData's slab)
        regs[r].rng = rngs[r]; regs[r].draw = vit_draw;
        regs[r].index = lockstep ? r : -1;
    }
    std::vector<std::vector<std::vector<int>>> paths;
    {
        // sub-batches of regions that fit this runtime's device share (obs, trimmed means, back-pointers and forward
        // probabilities: 26 KB per position; ~270 MB per 10 kb region); the regions' generators keep the results the same however
        // the batch is cut; a sub-batch the device has no memory for is cut in two
        auto need = [&](size_t k) { return 26.0 * 1024.0 * (double)regs[k].T + 32.0 * (double)regs[k].T * regs[k].E; };
        double cap = std::max(1e9, PLAN_VITERBI_FRAC * device_share_bytes());   // (the tables live in the runtime's matrix pool, which no alignment uses during this call)
        for (size_t k0 = 0; k0 < regs.size();) {
            size_t k1 = k0;
            double acc = 0;
            for (; k1 < regs.size(); k1++) { const double add = need(k1); if (k1 > k0 && acc + add > cap) break; acc += add; }
            std::vector<std::vector<std::vector<int>>> part;
            const int rc = viterbi_device_multi(rt, std::vector<VitRegionH>(regs.begin() + k0, regs.begin() + k1), nkeep, skip, stay, mmin, mmax, &part, tap, who);
            if (rc == PS_ERR_NOMEM && k1 - k0 > 1) { cap *= 0.5; continue; }   // (nothing of this sub-batch has been drawn yet: allocation comes first)
            PS_TRY(rc);
            for (auto& pr : part) paths.push_back(std::move(pr));
            k0 = k1;
        }
    }
    tk.lap("device");
    par_for(R, [&](int r) { for (auto& p : paths[r]) outs[r]->push_back(path_to_bases(p)); });
    tk.lap("paths to bases");
    return PS_OK;
}

int viterbi_mutate(Runtime* rt, Align* a, int nkeep, double skip, double stay, double mmin, double mmax,
                   std::vector<std::string>* out, bool verbose) {
    const int rc = viterbi_mutate_multi(rt, {a}, {nullptr}, nkeep, skip, stay, mmin, mmax, {out}, nullptr, "ps_viterbi_mutate", false);
    if (verbose && rc == PS_OK) {
        // the reference's progress line (cpp/Viterbi.cpp:258-259, 357-370): "Viterbi", a dot whenever the reference position passes a
        // multiple of 200, a newline.  The positions walked: from the first event's start to where no event is aligned any more —
        // counted here from the sequence length (the walk itself runs on the device)
        fputs("Viterbi", stderr);
        for (size_t k = 200; k <= a->bases.size(); k += 200) fputc('.', stderr);
        fputc('\n', stderr);
        fflush(stderr);
    }
    return rc;
}

}  // namespace ps
