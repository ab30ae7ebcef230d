// ps_sw.h — host API of the Smith-Waterman module: the kernels and sw_run in ps_sw.hip, everything else in ps_swhost.cpp; the pair
// record, the result record and the checkpoint layout in ps_swplan.h
#ifndef PS_SW_H_
#define PS_SW_H_
#include "ps_internal.h"
#include "ps_swplan.h"

namespace ps {

// a, b: list form only.  n_pairs, n_match: both forms.  first / last / gap: summary form only (entry 0, entry n_pairs - 1, entries == 0
// of inds1 / inds2; all 0 for an empty alignment).  map_*: map form only (RemapRec; map_off: the pair's table, in ints from the d_map
// the batch was given).
struct SwResult {
    int score = 0; double accuracy = 0; std::vector<int> a, b;
    int n_pairs = 0, n_match = 0, first1 = 0, first2 = 0, last1 = 0, last2 = 0, gap1 = 0, gap2 = 0;
    int map_lo = 0, map_hi = 0, map_has0 = 0, map_y0 = 0;
    int64_t map_off = 0;
};

// an enqueued batch: host staging stays alive until sw_finish
struct SwJob {
    std::vector<SwPair> pairs;
    std::string pool;
    int* res = nullptr;        // pinned host staging (runtime-owned): results and index pairs
    int* outbuf = nullptr;     // (list form only)
    int* d_map = nullptr;      // (map form only) device memory of the caller's for the pairs' tables: n1 + 2 ints each, in input order
    SwForm form = SW_LISTS;
    int64_t out_tot = 0;
    double cells = 0;
    double band_cells = 0;     // cells the fill computes (full-matrix pairs count n1 x n2)
    int np = 0;
    int nband = 0;             // pairs in band mode
    hipStream_t stream = nullptr;   // where the batch was enqueued
};

typedef std::vector<std::pair<const std::string*, const std::string*>> SwInput;
// band half-width for one pair under PORESEQ_SW_BAND (off / auto / force) and PORESEQ_SW_BAND_W; 0: the full matrix
int sw_band_choice(const std::string& s1, const std::string& s2);
// asynchronous, on the runtime's second stream (or its main one under load); wb: per-pair band half-widths (nullptr: sw_band_choice)
// (map form: job->d_map set by the caller before the launch)
int sw_launch(Runtime* rt, const SwInput& in, SwJob* job, const int* wb = nullptr, SwForm form = SW_LISTS);
int sw_finish(Runtime* rt, SwJob* job, std::vector<SwResult>* out);   // redoes the pairs whose band certificate failed on the full matrix, in the job's form
int sw_batch(Runtime* rt, const SwInput& in, std::vector<SwResult>* out, const int* wb = nullptr, SwForm form = SW_LISTS, int* d_map = nullptr);
int64_t sw_map_ints(const SwInput& in, size_t k0, size_t k1);   // ints the tables of pairs k0 .. k1 - 1 take in map form
// chunking by device memory, shared by FindMutations and the summary entry point: the cap of one launch, the end of the chunk that
// starts at pair k0, and the loop that runs pairs k0 .. end chunk by chunk (halving the cap on PS_ERR_NOMEM), appending to `out`
double sw_chunk_cap();
size_t sw_chunk_end(const SwInput& in, const int* wbs, SwForm form, size_t k0, double cap);
// (map form: d_map holds the tables of ALL pairs of `in`, sw_map_ints(in, 0, in.size()) ints; SwResult::map_off counts from it)
int sw_chunks(Runtime* rt, const SwInput& in, const int* wbs, SwForm form, size_t k0, std::vector<SwResult>* out, int* nchunks = nullptr, int* d_map = nullptr);
// any number of pairs in summary form (band choice per pair, chunked): ps_batch_sw_summary
int sw_summaries(Runtime* rt, const SwInput& in, std::vector<SwResult>* out);
void sw_band_counters(int64_t out[5]);   // cumulative: pairs banded, fell back, maxima near a band edge, band cells, full-matrix cells

// the device pointers of an enqueued batch
struct SwDev { const SwPair* pairs; const char* chars; int *row, *col, *blk, *prog, *ticket, *out, *res; };
// Fill and traceback (list, summary or map build, SwForm) of np pairs in one form: K columns per lane on `waves` waves per workgroup,
// chained over nss strips (sw_launch on why each exists).  packed: the 16-bit fill (8 columns per lane, SWW waves) with the traceback
// of the 8-column build; band: the packed fill, one workgroup of SWBW waves per pair over its 512-column strips, the same traceback
// (band-aware through SwPair::wb).  In ps_sw.hip: the one function that names the kernels.
int sw_run(hipStream_t st, const SwDev& d, int np, int nss, int K, int waves, bool packed, bool band, SwForm form);

}  // namespace ps
#endif
