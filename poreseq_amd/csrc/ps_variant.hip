// ps_variant.hip — `poreseq variant -v` (poreseq/Variant.py:48-61): score whole candidate sequences against the events of a region.
//
// The reference copies the AlignData per variant, re-maps every event onto the variant through swalign and PSEvent.mapaligns
// (_poreseqcpp.pyx:241-261, poreseq/EventData.py:226-256) and calls ScoreEvents.  Here all variants of all regions go through one chain:
//   Smith-Waterman of (current sequence, variant) in map form (ps_sw.hip, SW_MAP): per pair a partner table that stays on the device and
//     a small record — the one device-to-host copy before the scores (the band certificate needs the host anyway)
//   k_remap: every (variant, event) job's ref_align from the event's current one, the pair's table and record (ps_remap.h)
//   updaterefs, forward fills and backtrace of the jobs (realign), their maxima gathered into one array
// chunked by this runtime's share of the device like FindMutations' candidate sequences (fwd_chunk_end).  No index list, ref_align
// mirror or remapped alignment crosses PCIe, and the AlignData are only read.
#include <map>

#include "ps_host.h"
#include "ps_remap.h"
#include "ps_sw.h"

namespace ps {

// one (region, variant) unit of a chunk: `n` levels (all events of the region, as they lie in its slab) to re-map through one table
struct RemapUnit {
    const double* src;   // the events' current ref_align (AlignData slab)
    const int* part;     // the pair's partner table
    int64_t n;           // levels
    int64_t dst;         // into the chunk's job arrays
    RemapRec rec;
};

// grid (units, blocks of 256 levels): one thread per level of every (variant, event) job; ref_like starts cleared, as a fresh
// alignment's does (the fills rewrite it)
__global__ __launch_bounds__(256) void k_remap(const RemapUnit* __restrict__ units, double* __restrict__ ra, double* __restrict__ rl) {
    const RemapUnit u = units[blockIdx.x];   // (the unit in x: a chunk may hold more units than the 65 535 blocks y allows)
    for (int64_t t = (int64_t)blockIdx.y * blockDim.x + threadIdx.x; t < u.n; t += (int64_t)gridDim.y * blockDim.x) {
        ra[u.dst + t] = remap_level(u.src[t], u.part, u.rec);
        rl[u.dst + t] = 0.0;
    }
}

static int launch_remap(Runtime* rt, const std::vector<RemapUnit>& rus, double* d_ra, double* d_rl) {
    if (rus.empty()) return PS_OK;
    int64_t maxn = 1;
    for (const RemapUnit& u : rus) maxn = std::max(maxn, u.n);
    DBuf& ub = rt->buf("remap_units");
    PS_TRY(ub.ensure(rus.size() * sizeof(RemapUnit)));
    PS_TRY(rt->up(ub.p, rus.data(), rus.size() * sizeof(RemapUnit)));
    const unsigned by = (unsigned)std::min<int64_t>((maxn + 255) / 256, 1024);   // (longer units: the kernel strides)
    hipLaunchKernelGGL(k_remap, dim3((unsigned)rus.size(), by), dim3(256), 0, rt->stream, ub.as<RemapUnit>(), d_ra, d_rl);
    PS_LAUNCH_CHECK();
    if (rt->prof_on) rt->prof["remap"].launches++;
    return PS_OK;
}

int score_sequences_multi(Runtime* rt, const std::vector<Align*>& as, const std::vector<const std::vector<std::string>*>& seqs,
                          const std::vector<double*>& scores, const std::vector<double*>& accuracy) {
    Tick tk("score_sequences");
    const int R = (int)as.size();
    // units: the distinct variant strings of every region (identical ones are aligned and scored once)
    struct Unit { int r, s; std::vector<int> states; };
    std::vector<Unit> units;
    std::vector<std::vector<int>> unit_of(R);   // [region][variant] -> unit
    for (int r = 0; r < R; r++) {
        std::map<std::string, int> seen;
        const std::vector<std::string>& sv = *seqs[r];
        unit_of[r].resize(sv.size());
        for (int s = 0; s < (int)sv.size(); s++) {
            auto it = seen.find(sv[s]);
            if (it == seen.end()) { it = seen.emplace(sv[s], (int)units.size()).first; units.push_back({r, s, {}}); }
            unit_of[r][s] = it->second;
        }
    }
    if (units.empty()) return PS_OK;
    const size_t U = units.size();
    // Smith-Waterman of every current sequence against each of its variants (swalign(self.sequence, newseq), pyx:253): the tables of all
    // pairs in one buffer (n1 + 2 ints each), launches cut by the Smith-Waterman share of the device
    SwInput pairs(U);
    for (size_t u = 0; u < U; u++) pairs[u] = {&as[units[u].r]->bases, &(*seqs[units[u].r])[units[u].s]};
    std::vector<int> wbs(U);
    for (size_t u = 0; u < U; u++) wbs[u] = sw_band_choice(*pairs[u].first, *pairs[u].second);
    DBuf& mb = rt->buf("var_map");
    PS_TRY(mb.ensure((size_t)sw_map_ints(pairs, 0, U) * sizeof(int)));
    std::vector<SwResult> als;
    int sw_nchunks = 0;
    PS_TRY(sw_chunks(rt, pairs, wbs.data(), SW_MAP, 0, &als, &sw_nchunks, mb.as<int>()));
    tk.lap("smith-waterman (map form)");
    for (size_t u = 0; u < U; u++)
        if (als[u].n_pairs <= 0)   // (the reference dies here: IndexError on an empty pairs array, EventData.py:250)
            return fail(PS_ERR_BAD_ARG, "score_sequences: sequence " + std::to_string(units[u].s) + (R > 1 ? " of region " + std::to_string(units[u].r) : std::string()) +
                                        " has no alignment with the current sequence");
    for (int r = 0; r < R; r++)
        if (accuracy[r]) for (size_t s = 0; s < seqs[r]->size(); s++) accuracy[r][s] = als[unit_of[r][s]].accuracy;
    // (region, variant) units with events get (variant x event) forward-only jobs
    std::vector<size_t> live;
    for (size_t u = 0; u < U; u++) if (as[units[u].r]->E) live.push_back(u);
    par_for((int)live.size(), [&](int q) { Unit& un = units[live[q]]; un.states = states_of((*seqs[un.r])[un.s]); });
    std::vector<FwdUnit> fu(live.size());
    for (size_t q = 0; q < live.size(); q++) fu[q] = {as[units[live[q]].r], (int)units[live[q]].states.size()};
    std::vector<std::vector<double>> best_of(U);   // per unit: E scores
    const double cap = fwd_chunk_cap();
    size_t q0 = 0, limit = (size_t)-1;
    int p_seen = 0, nchunks = 0;
    while (q0 < live.size()) {
        size_t nref = 0;
        const size_t q1 = fwd_chunk_end(fu, q0, cap, p_seen, limit, &nref);
        const size_t stage_mark = rt->stage.mark();
        DBuf& rb = rt->buf("seed_refs");
        PS_TRY(rb.ensure((size_t)3 * std::max<size_t>(nref, 1) * sizeof(double)));
        double* d_ra = rb.as<double>();
        double* d_rl = d_ra + nref;
        double* d_ri = d_rl + nref;
        std::vector<RemapUnit> rus(q1 - q0);
        std::vector<size_t> roff(q1 - q0 + 1, 0);
        size_t njobs = 0;
        for (size_t q = q0; q < q1; q++) {
            const Align* a = fu[q].a;
            const SwResult& al = als[live[q]];
            roff[q - q0 + 1] = roff[q - q0] + (size_t)a->ntot;
            rus[q - q0] = {a->d_ra, mb.as<int>() + al.map_off, a->ntot, (int64_t)roff[q - q0], {al.map_lo, al.map_hi, al.map_has0, al.map_y0}};
            njobs += a->E;
        }
        PS_TRY(launch_remap(rt, rus, d_ra, d_rl));
        DBuf& ob = rt->buf("seed_out");
        PS_TRY(ob.ensure(njobs * sizeof(JobOut)));   // (before the out pointers are taken: ensure() may move the buffer)
        PS_HIP(hipMemsetAsync(ob.p, 0, njobs * sizeof(JobOut), rt->stream));
        std::vector<JobSpec> specs;
        for (size_t q = q0; q < q1; q++) {
            Align* a = as[units[live[q]].r];
            for (int e = 0; e < a->E; e++) {
                JobSpec s = a->job(e);   // the event's data; the variant's states and its re-mapped alignment on top
                s.states = &units[live[q]].states;
                const size_t o = roff[q - q0] + a->off[e];
                s.ra = d_ra + o; s.rl = d_rl + o; s.ri = d_ri + o;
                s.out = ob.as<JobOut>() + specs.size();
                specs.push_back(s);
            }
        }
        Batch b;
        PS_TRY(b.build(rt, specs, 1, 0));
        PS_TRY(launch_updaterefs(rt, b.d));   // EventData::setData of the copy's AlignData ends with updaterefs (cpp/EventData.h:223)
        {
            const int rc = realign(rt, b, q1 - q0 > 1 ? PLAN_OVER_GUESS * cap : 0.0);
            if (rc == PS_SPLIT) {   // wider bands than guessed: cut the chunk again with the width it asked for
                if (trace_on()) fprintf(stderr, "[ps] variant chunk of %zu cut again: %d slots per anti-diagonal\n", q1 - q0, b.P);
                p_seen = std::max(p_seen, b.P);
                limit = std::max<size_t>(1, (q1 - q0) / 2);
                PS_HIP(hipStreamSynchronize(rt->stream));
                rt->stage.release(stage_mark);
                continue;
            }
            PS_TRY(rc);
        }
        p_seen = std::max(p_seen, b.P);
        double* best = nullptr;
        DBuf& gb = rt->buf("best");
        PS_TRY(gb.ensure(specs.size() * sizeof(double)));
        PS_TRY(launch_gather_best(rt, b.d, gb.as<double>()));
        PS_TRY(rt->down(&best, gb.p, specs.size()));
        PS_HIP(hipStreamSynchronize(rt->stream));
        size_t j = 0;
        for (size_t q = q0; q < q1; q++) {
            std::vector<double>& v = best_of[live[q]];
            v.resize(fu[q].a->E);
            for (double& x : v) x = std::max(best[j++], 0.0);   // Alignment::getMax, cpp/Alignment.h:127-130
        }
        rt->stage.release(stage_mark);   // the stream is idle: this chunk's staging memory can be reused
        nchunks++;
        q0 = q1;
    }
    if (rt->prof_on) { Prof& pr = rt->prof["variant_chunks"]; pr.launches += nchunks; pr.units += (double)U; }
    if (trace_on()) fprintf(stderr, "[ps] score_sequences: %zu distinct sequences of %d regions, %d smith-waterman launches, %d alignment chunks\n", U, R, sw_nchunks, nchunks);
    tk.lap("remap + realign");
    for (int r = 0; r < R; r++) {
        const int E = as[r]->E;
        for (size_t s = 0; s < seqs[r]->size() && E; s++) {
            const std::vector<double>& v = best_of[unit_of[r][s]];
            std::copy(v.begin(), v.end(), scores[r] + s * (size_t)E);
        }
    }
    return PS_OK;
}

}  // namespace ps
