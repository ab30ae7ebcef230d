// ps_find.cpp — FindMutations (cpp/FindMutations.cpp:24-186), MapAlignments (cpp/EventUtil.cpp:12-55) and
// fillinds (cpp/swlib.cpp:342-365).  The alignments and the Smith-Waterman matrices run on the GPU; what is left
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

}  // namespace ps
