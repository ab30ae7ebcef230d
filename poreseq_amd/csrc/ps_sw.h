// ps_sw.h — host-visible types of the Smith-Waterman module (ps_sw.hip)
#ifndef PS_SW_H_
#define PS_SW_H_
#include "ps_internal.h"

namespace ps {

struct SwPair {
    int n1, n2;                  // rows (first sequence), columns (second sequence)
    int nrb;                     // row blocks of 64
    int ngw;                     // wave strips (16 per super-strip)
    int pitch;                   // ints per saved row
    int wb;                      // band half-width (a multiple of 64; 0: the full matrix)
    int nbb;                     // band mode: row blocks of 64 kept per 512-column strip (8 + 2 wb / 64)
    int cpitch;                  // ints per saved column: n1 + 1, band mode 64 nbb + 1
    int64_t s1_off, s2_off;      // into the character pool
    int64_t row_off;             // rowsave: nrb x pitch ints, row q = H(64q, 1..n2) at [0..n2)  (band: strips x nbb x 512)
    int64_t col_off;             // colsave: (n2/64 + 1) x cpitch ints, entry c = H(0..n1, 64c)  (c = 0 unused: zeros)
    int64_t blk_off;             // blkmax: nrb x ngw ints  (band: strips x nbb)
    int64_t out_off;             // 2 * (n1 + n2 + 2) ints: index pairs in walk order; map form: n1 + 2 ints, the partner table part[i1] = i2
    int64_t res_off;             // SW_RES ints: score, bi, bj, npairs, nmatch, timed out, band certificate failed, -; summary form: first1,
                                 // first2, last1, last2, gap1, gap2 (the ends of the reversed index lists and their zero entries);
                                 // map form: lo, hi, has0, y0 (RemapRec, ps_remap.h)
};
constexpr int SW_RES = 16;       // ints per result record

// what the traceback leaves: the index lists (swfull, cpp/swlib.cpp:279-333), or only what a caller reads off them (first and last
// aligned pair, gap counts) in one fixed record per pair, with no list buffer on the device, no staging and no copy of one; or what
// PSEvent.mapaligns makes of the lists (ps_remap.h): per pair a table part[i1] = i2 over seq1 (0 where the base faces a gap) that STAYS
// on the device, in a buffer of the caller's (SwJob::d_map), and a four-int record about it
enum SwForm { SW_LISTS = 0, SW_SUMMARY = 1, SW_MAP = 2 };

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
double sw_pair_bytes(int n1, int n2, int wb, SwForm form = SW_LISTS);   // device bytes of one pair's checkpoints and (list form) index lists
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

}  // namespace ps
#endif
