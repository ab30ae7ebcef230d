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
    int64_t out_off;             // 2 * (n1 + n2 + 2) ints: index pairs in walk order
    int64_t res_off;             // 8 ints: score, bi, bj, npairs, nmatch, timed out, band certificate failed
};

struct SwResult { int score = 0; double accuracy = 0; std::vector<int> a, b; };

// an enqueued batch: host staging stays alive until sw_finish
struct SwJob {
    std::vector<SwPair> pairs;
    std::string pool;
    int* res = nullptr;        // pinned host staging (runtime-owned): results and index pairs
    int* outbuf = nullptr;
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
double sw_pair_bytes(int n1, int n2, int wb);   // device bytes of one pair's checkpoints and index lists
// asynchronous, on the runtime's second stream (or its main one under load); wb: per-pair band half-widths (nullptr: sw_band_choice)
int sw_launch(Runtime* rt, const SwInput& in, SwJob* job, const int* wb = nullptr);
int sw_finish(Runtime* rt, SwJob* job, std::vector<SwResult>* out);   // redoes the pairs whose band certificate failed on the full matrix
int sw_batch(Runtime* rt, const SwInput& in, std::vector<SwResult>* out, const int* wb = nullptr);
void sw_band_counters(int64_t out[5]);   // cumulative: pairs banded, fell back, maxima near a band edge, band cells, full-matrix cells

}  // namespace ps
#endif
