// ps_ownplan.h — where the outputs of an own-sequence statistics call (ps_own.cpp) lie in "astats", on plain data: the one statement
// of it.  The descriptors point there, the one copy back reads from there, the scatter into the callers' arrays takes its addresses
// from there.  No HIP headers (tests/native/ownplan_check.cpp compiles this text with g++ and holds every offset to a restatement).
#ifndef PS_OWNPLAN_H_
#define PS_OWNPLAN_H_
#include <algorithm>
#include <cstdint>
#include <vector>
#include "../../include/poreseq_hip.h"

namespace ps {
enum class OwnKind { Score, AlignStats, KmerStats, MoveStats, Posterior };   // (ps_host.h says what each computes)

// A call as the plan sees it.  levels: the region wants a per-level array (MoveStats: step or col, Posterior: emit and col);
// ngroups: KmerStats; C, W: the job's states and band half-width (the posterior call's cell count)
struct OwnView {
    OwnKind kind = OwnKind::Score;
    bool re = false;   // a realignment runs: the scores come back too
    struct Region { int E = 0, ngroups = 0; bool levels = false; };
    struct Job { int n0 = 0, C = 0, W = 0; };
    std::vector<Region> regs; std::vector<Job> jobs;   // jobs: of all regions, in order
};

// The outputs, in their order in the buffer: the records (ps_event_stats / ps_event_moves / ps_event_posterior, one per job) or the
// tables (ps_kmer_cell, PS_N_STATES per group); the scores; MoveStats' columns and step codes, Posterior's emit and col (one entry
// per level of every job, for all jobs once a region wants them); the posterior kernels' per-row sums (eight doubles per level),
// which do not come back
enum OwnOut { OO_MAIN, OO_SCORES, OO_COL, OO_STEP, OO_EMIT, OO_PCOL, OO_ROW, OO_COUNT };

struct OwnPlan {
    size_t nj = 0, levels = 0, rows = 0;   // jobs, their levels, table rows
    bool per_level = false; int maxE = 0, maxG = 0;   // most events / groups of one region
    size_t at[OO_COUNT] = {}, bytes[OO_COUNT] = {};
    size_t back_bytes = 0, ensure_bytes = 0;   // what the one copy returns; with the scratch behind it
    std::vector<size_t> lev_off;           // [job] its first level in the per-level outputs
    std::vector<int> job0, tab0;           // [region] its first job and first table row
    double alg_bytes = 0.0;                // for the profile: algorithmic bytes of the reduction; Posterior: its band cells
    // output o in a buffer at `base`: entry i of it, and the first of job q's levels (`per` entries each)
    template <class T> T* item(const void* base, OwnOut o, size_t i = 0) const { return (T*)((char*)base + at[o]) + i; }
    template <class T> T* level(const void* base, OwnOut o, size_t q, size_t per = 1) const { return item<T>(base, o, lev_off[q] * per); }
};

inline size_t own_out_elem(OwnKind kind, OwnOut o) {
    if (o == OO_MAIN)
        return kind == OwnKind::AlignStats ? sizeof(ps_event_stats) : kind == OwnKind::KmerStats ? sizeof(ps_kmer_cell) :
               kind == OwnKind::MoveStats ? sizeof(ps_event_moves) : kind == OwnKind::Posterior ? sizeof(ps_event_posterior) : 0;
    return o == OO_COL ? sizeof(int32_t) : o == OO_STEP ? sizeof(uint8_t) : sizeof(double);
}
// bytes of output o of a call whose counts are in p; 0: the call has none (Score has none at all: its scores go through "best")
inline size_t own_out_bytes(const OwnView& v, const OwnPlan& p, OwnOut o) {
    const bool moves = v.kind == OwnKind::MoveStats, post = v.kind == OwnKind::Posterior;
    size_t count = 0;
    switch (o) {
    case OO_MAIN: count = v.kind == OwnKind::KmerStats ? p.rows * PS_N_STATES : p.nj; break;
    case OO_SCORES: count = v.re && !post && v.kind != OwnKind::Score ? p.nj : 0; break;
    case OO_COL: case OO_STEP: count = moves && p.per_level ? p.levels : 0; break;
    case OO_EMIT: case OO_PCOL: count = post && p.per_level ? p.levels : 0; break;
    case OO_ROW: count = post ? p.levels * 8 : 0; break;
    case OO_COUNT: break;
    }
    return count * own_out_elem(v.kind, o);
}

inline OwnPlan lay_out(const OwnView& v) {
    OwnPlan p;
    const bool kmer = v.kind == OwnKind::KmerStats;
    for (const OwnView::Region& r : v.regs) {
        p.job0.push_back((int)p.nj); p.tab0.push_back((int)p.rows);
        p.nj += (size_t)r.E; p.rows += kmer ? (size_t)r.ngroups : 0;
        p.maxE = std::max(p.maxE, r.E); p.maxG = std::max(p.maxG, kmer ? r.ngroups : 0);
        p.per_level |= r.levels;
    }
    for (const OwnView::Job& j : v.jobs) {
        p.lev_off.push_back(p.levels); p.levels += (size_t)j.n0;
        if (v.kind == OwnKind::Posterior) p.alg_bytes += (double)j.C * std::min<double>(2.0 * j.W + 1, j.n0);
    }
    for (int o = 0; o < OO_COUNT; o++) {
        if (o == OO_ROW) p.back_bytes = p.ensure_bytes;
        p.at[o] = p.ensure_bytes; p.bytes[o] = own_out_bytes(v, p, (OwnOut)o); p.ensure_bytes += p.bytes[o];
    }
    if (v.kind != OwnKind::Posterior && v.kind != OwnKind::Score)
        p.alg_bytes = (kmer ? 24.0 : v.kind == OwnKind::AlignStats ? 16.0 : p.per_level ? 13.0 : 8.0) * (double)p.levels + (double)p.bytes[OO_MAIN];
    return p;
}
}  // namespace ps
#endif
