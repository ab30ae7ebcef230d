// ps_poison.h — what ps_debug_poison (ps_mem.cpp) writes into each named pool of a runtime.  Host-only, no HIP.
//
// Pools, slabs, cached slabs and staging memory are scratch between API calls: the hook overwrites them so
// that a kernel or host loop that reads what its own call did not write gets a pattern instead of zeros or a neighbour's scores.
//   INDEX   the 32-bit index word in every word.  The default, and the class of every buffer a consumer — device or host — may
//           turn into an address, offset, count, flag, state id or loop bound: the tests pass 1, nonzero and in range wherever it
//           is used that way, so that a stale read gives a wrong result and never a stray address.
//   VALUE   the 64-bit value word in every double.  Only for buffers whose content is compared, added and copied and nothing
//           else; every such entry says why.
//   EXEMPT  carries state from one call to the next on purpose: left alone and reported as skipped.  (None today.)
// Every name that csrc passes to Runtime::buf() or Runtime::hbuf() has one line here; tests/test_poison_table.py holds the two
// sets equal.  The pinned host buffers of the same names, the staging arena, the dense slabs (records and step words, like
// "rec" and "flg") and the cached AlignData slabs (events, states, JobOut) always get the index word.
//
// What the index word does not show: in "rec" and the dense slabs, the largest buffers, two words of 1 read as the double
// 2.1e-314, which a max or a sum treats like the zero of a fresh allocation.  The constant patterns therefore do not cover stale
// reads of DP records; only leftovers of a real call do (tests/test_hip_poison.py, the large region right before the small one).
#ifndef PS_POISON_H_
#define PS_POISON_H_

#include <cstring>

namespace ps {

enum class PoisonClass { INDEX = 0, VALUE = 1, EXEMPT = 2 };
struct PoisonEntry { const char* name; PoisonClass cls; const char* why; };

constexpr PoisonEntry POISON_TABLE[] = {
    // the DP batch (ps_host.cpp, ps_own.cpp, ps_mem.cpp, ps_kernels.hip)
    {"jobs", PoisonClass::INDEX, "JobD: pointers, sizes, offsets"},
    {"states", PoisonClass::INDEX, "5-mer state ids and their -1 padding"},
    {"lb", PoisonClass::INDEX, "band centres per column"},
    {"lo", PoisonClass::INDEX, "lowest in-band row per anti-diagonal"},
    {"hi", PoisonClass::INDEX, "highest in-band row per anti-diagonal"},
    {"maxw", PoisonClass::INDEX, "widest footprint: sizes P"},
    {"fill_pairs", PoisonClass::INDEX, "job indices of paired fills"},
    {"rec", PoisonClass::INDEX, "records {main, stay} — and the Viterbi arena, whose back-pointer shorts the host follows as state ids (vit_follow_bp)"},
    {"flg", PoisonClass::INDEX, "step words and strip codes: the backtrace turns them into moves"},
    {"cmax", PoisonClass::VALUE, "per-column maxima of main: read by k_prefix and the edit kernels as max operands only"},
    {"pm", PoisonClass::VALUE, "prefix maxima over columns: compared and added, never indexed with"},
    {"best", PoisonClass::VALUE, "JobOut.best gathered per job: copied to the host and clamped at 0"},
    // strip sweeps (ps_sweep.hip)
    {"sw_jobs", PoisonClass::INDEX, "SweepJob: offsets and step counts"},
    {"sw_band", PoisonClass::INDEX, "row bounds per column"},
    {"sw_qlo", PoisonClass::INDEX, "lowest strip in band per step"},
    {"sw_qhi", PoisonClass::INDEX, "highest strip in band per step"},
    {"sw_sb", PoisonClass::INDEX, "StripBest: score with its cell"},
    {"sw_win", PoisonClass::INDEX, "widest window of strips: sizes the launch"},
    // Smith-Waterman (ps_swhost.cpp)
    {"sw_pairs", PoisonClass::INDEX, "SwPair: lengths and offsets"},
    {"sw_chars", PoisonClass::INDEX, "sequence bytes, compared and used as substitution keys"},
    {"sw_row", PoisonClass::INDEX, "checkpoint rows of packed scores and directions"},
    {"sw_col", PoisonClass::INDEX, "checkpoint columns"},
    {"sw_blk", PoisonClass::INDEX, "block maxima with their cells"},
    {"sw_prog", PoisonClass::INDEX, "progress counters the blocks spin on"},
    {"sw_out", PoisonClass::INDEX, "index lists"},
    {"sw_res", PoisonClass::INDEX, "per-pair records: score, cell, list length"},
    {"sw_map_redo", PoisonClass::INDEX, "position tables of redone pairs"},
    // candidate alignments (ps_fwd.cpp, ps_find.cpp, ps_variant.hip)
    {"seed_refs", PoisonClass::INDEX, "ref_align doubles are converted to column indices"},
    {"seed_out", PoisonClass::INDEX, "JobOut: cells and flags beside the score"},
    {"like_groups", PoisonClass::INDEX, "LikeGroup: job ranges and offsets"},
    {"like_out", PoisonClass::VALUE, "per-base likelihood sums: copied to the host and differenced"},
    {"remap_units", PoisonClass::INDEX, "unit descriptors of k_remap"},
    {"var_map", PoisonClass::INDEX, "position tables"},
    // edit scoring (ps_score.cpp)
    {"keep", PoisonClass::INDEX, "kept-column index per column"},
    {"mutint", PoisonClass::INDEX, "edit tables and descriptors"},
    {"mutdbl", PoisonClass::VALUE, "old / delta / score / oldall doubles: max and sum operands, copied to the host as scores"},
    {"ptable", PoisonClass::INDEX, "ps_point_best carries slots beside the scores"},
    {"support", PoisonClass::INDEX, "records with counts"},
    {"phase", PoisonClass::INDEX, "links, set ids, haplotype tags"},
    // alignment census and k-mer statistics (ps_own.cpp)
    {"astats_in", PoisonClass::INDEX, "StatJob / StatRegion: pointers and sizes"},
    {"astats", PoisonClass::INDEX, "ps_event_stats and ps_kmer_cell carry counts"},
    // Viterbi (placed by viterbi_batch, ps_vit.cpp; the kernels: ps_viterbi.hip)
    {"vit_regs", PoisonClass::INDEX, "VitReg: pointers, sizes, offsets"},
    {"vit_posreg", PoisonClass::INDEX, "region of every position"},
    {"vit_in", PoisonClass::INDEX, "the fourth double of every record is the `present` flag"},
    {"vit_lik", PoisonClass::VALUE, "final scores per state: the host takes their argmax, a comparison of values"},
    {"vit_att", PoisonClass::INDEX, "default"},
    {"vit_start", PoisonClass::INDEX, "start state of the traces"},
    {"vit_rnd", PoisonClass::INDEX, "deviates: the picked state depends on them"},
    {"vit_path", PoisonClass::INDEX, "state paths"},
};

inline const PoisonEntry* poison_entry(const char* name) {
    for (const PoisonEntry& e : POISON_TABLE) if (!strcmp(e.name, name)) return &e;
    return nullptr;
}

}  // namespace ps

#endif
