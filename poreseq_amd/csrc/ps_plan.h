// ps_plan.h — the arithmetic of the device-memory plan: pure, host-only, no HIP include.  Shared by the library (ps_mem.cpp decides
// with it, ps_host.cpp, ps_own.cpp, ps_fwd.cpp and ps_vit.cpp size their batches with it) and by a host test of it (tests/native/plan_check.cpp).
//
// The plan (309 GB on an MI355X, or this process's fraction of it):
//   27 %  three slabs of 9 % each for the full forward + backward score matrices of dense ScoreMutations calls
//   13 %  left alone: the HSA runtime aborts the process when a launch finds no memory for its own needs, and hipMalloc rounds
//         (pools that summed to 302 GB left 5 GB free)
//   60 %  the runtimes, one per host thread inside the library.  What a runtime holds follows its share: the matrix pool grows
//         6 % past it, small forward batches (k_fill) add an eighth in step words, Smith-Waterman checkpoints a quarter, and
//         ~2.5 GB do not depend on it (remapped alignments, band tables, edit tables): 1.4 x share + 2.5 GB, measured at 7, 10 and
//         14 batches in flight.  So share = (0.60 x device / threads - 2.5 GB) / 1.4 with at least four threads:
//         31 GB up to four threads, 17 GB at seven, 7.7 GB at fourteen.
// The share sizes the chunks of FindMutations' candidate alignments (7 MB of step codes each), of Smith-Waterman batches and of
// the Viterbi tables.  Callers size their batches on a guess of the band footprint (guess_slots_w) and split when realign() finds
// the matrices 20 % over the share, or the device short of memory.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace ps {

// ---- the share of one runtime ----------------------------------------------------------------------------------------------
constexpr double PLAN_RUNTIMES_FRAC = 0.60;   // of the device: all runtimes together
constexpr double PLAN_PER_SHARE = 1.4;        // bytes a runtime holds per byte of its share ...
constexpr double PLAN_FIXED_BYTES = 2.5e9;    // ... plus what does not depend on the share
constexpr double PLAN_SHARE_FLOOR = 2e9;      // no share below this, however many threads
constexpr int PLAN_MIN_RUNTIMES = 4;          // the device is divided by at least this many: a lone thread's pools leave room for three more
constexpr double PLAN_OVER_GUESS = 1.2;       // realign()'s cap for a batch sized on a guess: the real matrices may come out a fifth over the share
constexpr int PLAN_SW_PART = 8;               // Smith-Waterman checkpoints: at most an eighth of the share per launch
constexpr double PLAN_VITERBI_FRAC = 0.9;     // Viterbi tables: all of the matrix pool but a tenth (no alignment uses it during that call)
constexpr double PLAN_VITERBI_FLOOR = 1e9;    // ... and no sub-batch of them is cut below this, however small the share

// ---- ceilings of the pools' sum (all runtimes + slabs), of this process's part of the device ----------------------------------
constexpr double PLAN_POOL_CEILING = 0.94;    // no buffer grows into the last 6 %: PS_ERR_NOMEM instead of the HSA runtime's abort
constexpr double PLAN_MATRIX_CEILING = 0.92;  // no matrix pool into the last 8 %: small buffers of every runtime live there

// ---- slabs for full score matrices, AlignData slab cache --------------------------------------------------------------------
constexpr double PLAN_SLAB_FRAC = 0.09;       // of the device each: 28 GB on an MI355X = the matrices of 10 regions per launch
constexpr int PLAN_SLABS = 3;
constexpr double PLAN_ALIGN_CACHE_FRAC = 0.03;   // cached AlignData slabs: at most 3 % of the device ...
constexpr double PLAN_ALIGN_CACHE_MAX = 8e9;     // ... and at most 8 GB

inline double share_bytes(size_t plan_bytes, int runtimes) {
    const int nrt = std::max(PLAN_MIN_RUNTIMES, runtimes);
    return std::max(PLAN_SHARE_FLOOR, (PLAN_RUNTIMES_FRAC * (double)plan_bytes / nrt - PLAN_FIXED_BYTES) / PLAN_PER_SHARE);
}
inline size_t slab_default_bytes(size_t plan_bytes) { return (size_t)(PLAN_SLAB_FRAC * (double)plan_bytes); }
inline size_t align_cache_default(size_t plan_bytes) { return std::min<size_t>((size_t)PLAN_ALIGN_CACHE_MAX, (size_t)(PLAN_ALIGN_CACHE_FRAC * (double)plan_bytes)); }

// ---- skewed score matrices (k_fill; layout in ps_internal.h) ----------------------------------------------------------------
constexpr int MAT_FRONT = 8;   // spare anti-diagonals in front of every matrix (the fill pipeline starts 8 steps early)
constexpr int MAT_BACK = 16;   // and behind it (the last loop body runs past S)
constexpr int PS_CELL_BYTES = 16 + 2;   // sizeof(double2) {main, stay} + sizeof(unsigned short) step word

// cells of one matrix of S = n0 + C + 1 anti-diagonals at P slots each
inline int64_t matrix_cells(int64_t S, int P) { return (S + MAT_FRONT + MAT_BACK) * P; }
// bytes of the matrices of one job in `ndir` directions.  Every factor is an integer far below 2^53 and so is the product (at most
// about 60 000 x 2048 x 36): exact in double, in any order of multiplication
inline double matrix_bytes(int64_t S, int P, int ndir) { return (double)matrix_cells(S, P) * PS_CELL_BYTES * ndir; }

// slots per anti-diagonal a band of half-width W will probably need: footprint ~ (2W + 1) / 1.9 for about one level per base, + 9
inline int guess_slots_w(int W) { return std::min(1024, std::max(64, (((2 * W + 1) * 10 / 19 + 9 + 63) / 64) * 64)); }
// and the most it can need while one slot per lane will do: the whole band 2W + 1, + 9 idle slots, rounded up to 64
inline int most_slots_w(int W) { return std::min(1024, 2 * W + 74); }

// Where the sub-batch that starts at item k0 of n ends when item k takes need(k) bytes and `cap` are to be had: everything if it
// fits; otherwise the list is cut into the fewest sub-batches that fit, of about equal size (a remainder of two regions behind two
// full sub-batches would cost a whole launch's latency for a tenth of the work).  An item larger than `cap` goes alone.
template <class Need> size_t share_cut(size_t k0, size_t n, double cap, Need&& need) {
    double total = 0;
    for (size_t k = k0; k < n; k++) total += need(k);
    if (total <= cap) return n;
    const double target = total / std::ceil(total / cap);      // bytes per sub-batch, all about equal
    double bytes = 0;
    size_t k = k0;
    for (; k < n; k++) {
        const double add = need(k);
        if (k > k0 && (bytes + add > cap || bytes + 0.5 * add > target)) break;
        bytes += add;
    }
    return k;
}

// Where the chunk that starts at item q0 of n ends when nothing is to be balanced: as many items, in order, as `cap` bytes hold, at
// most `limit` of them, always at least one (an item larger than `cap` goes alone).  The chunks of candidate-sequence alignments
// (fwd_chunks, ps_fwd.cpp): share_cut would move their boundaries.
template <class Need> size_t greedy_cut(size_t q0, size_t n, double cap, size_t limit, Need&& need) {
    size_t q1 = q0;
    double bytes = 0;
    while (q1 < n) {
        const double add = need(q1);
        if (q1 > q0 && (bytes + add > cap || q1 - q0 >= limit)) break;
        bytes += add; q1++;
    }
    return q1;
}

}  // namespace ps
