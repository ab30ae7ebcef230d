// ps_variant.hip — `poreseq variant -v` (poreseq/Variant.py:48-61): score whole candidate sequences against the events of a region.
//
// The reference copies the AlignData per variant, re-maps every event onto the variant through swalign and PSEvent.mapaligns
// (_poreseqcpp.pyx:241-261, poreseq/EventData.py:226-256) and calls ScoreEvents.  Here all variants of all regions go through one chain:
//   Smith-Waterman of (current sequence, variant) in map form (ps_sw.hip, SW_MAP): per pair a partner table that stays on the device and
//     a small record — the one device-to-host copy before the scores (the band certificate needs the host anyway)
//   k_remap: every (variant, event) job's ref_align from the event's current one, the pair's table and record (ps_remap.h)
//   updaterefs, forward fills and backtrace of the jobs (realign), their maxima gathered into one array
// chunked by this runtime's share of the device like FindMutations' candidate sequences (fwd_chunks, ps_fwd.cpp).  No index list, ref_align
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
    for (size_t q = 0; q < live.size(); q++) fu[q] = {as[units[live[q]].r], &units[live[q]].states};
    std::vector<std::vector<double>> best_of(U);   // per unit: E scores
    int nchunks = 0;
    auto place = [&](FwdChunk& c) -> int {   // every job's ref_align through its pair's table, on the device
        std::vector<RemapUnit> rus(c.q1 - c.q0);
        for (size_t q = c.q0; q < c.q1; q++) {
            const Align* a = fu[q].a;
            const SwResult& al = als[live[q]];
            rus[q - c.q0] = {a->d_ra, mb.as<int>() + al.map_off, a->ntot, (int64_t)c.roff[q - c.q0], {al.map_lo, al.map_hi, al.map_has0, al.map_y0}};
        }
        return launch_remap(rt, rus, c.d_ra, c.d_rl);
    };
    auto collect = [&](FwdChunk& c) -> int {   // the jobs' maxima
        double* best = nullptr;
        PS_TRY(gather_best(rt, c.b, &best));
        PS_HIP(hipStreamSynchronize(rt->stream));
        size_t j = 0;
        for (size_t q = c.q0; q < c.q1; q++) {
            std::vector<double>& v = best_of[live[q]];
            v.resize(fu[q].a->E);
            for (double& x : v) x = std::max(best[j++], 0.0);   // Alignment::getMax, cpp/Alignment.h:127-130
        }
        return PS_OK;
    };
    PS_TRY(fwd_chunks(rt, fu, "variant", place, collect, &nchunks));
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
