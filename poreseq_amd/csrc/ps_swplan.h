// ps_swplan.h — the checkpoint layout of the Smith-Waterman module, in one place: geometry constants, the pair record, the names of the
// result record's ints, the address of every rowsave / colsave / blkmax entry, and the host arithmetic that places a pair in the five
// pools.  Host and device, no HIP header: the fills and the traceback (ps_sw.hip) write and read through these functions, sw_launch
// (ps_swhost.cpp) sizes its buffers with sw_lay_out, and tests/native/sw_layout_check.cpp and sw_band_check.cpp compile this text with g++.
//
// The fill keeps, per pair,
//   rowsave  H(64q, *)    every 64th row       (top boundaries of 64-row blocks)
//   colsave  H(*, 64c)    every 64th column    (left boundaries of 64-column blocks)
//   blkmax   max H per (row block, wave strip)
// and the traceback recomputes the 64 x 64 tiles its path crosses from them.  A wave strip is the 64 K columns of one wave (K columns
// per lane); `waves` of them make one workgroup's super-strip.
// Band mode (SwPair::wb > 0): strips of SWBS columns, one wave each; strip s keeps only row blocks band_lo(s) .. band_lo(s) + nbb - 1
// (those inside 0 .. nrb - 1), i.e. rows [512 s + 1 - wb, 512 s + 512 + wb] rounded to whole blocks; every cell outside counts as 0.
#ifndef PS_SWPLAN_H_
#define PS_SWPLAN_H_

#include <stdint.h>
#include <stdlib.h>

#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PS_SW_HD __host__ __device__
#else
#define PS_SW_HD
#endif

namespace ps {

// ---- geometry -----------------------------------------------------------------------------------------------------------------
constexpr int SWB = 8;               // rows per pipeline step
constexpr int SWW = 8;               // waves per workgroup of the chained form: two per SIMD keeps one pair's strips issue-balanced over several CUs
constexpr int SWW1 = 16;             // waves per workgroup of the one-workgroup-per-pair form
constexpr int SWBS = 512;            // columns per strip of the band mode (one wave of 64 lanes x 8 columns)
constexpr int SWBW = 4;              // waves per pair in band mode (one strip each at a time)
constexpr int PKK = 8;               // columns per lane of the packed 16-bit fill
constexpr int SW_PK_MAXLEN = 13000;  // the packed fill's longest pair: 5 x 13 000 + 8 x 9 + 13 < 65 536
constexpr int SW_BAND_W = 1024;      // default band half-width
constexpr int SW_RES = 16;           // ints per result record

// what the traceback leaves: the index lists (swfull, cpp/swlib.cpp:279-333), or only what a caller reads off them (first and last
// aligned pair, gap counts) in one fixed record per pair, with no list buffer on the device, no staging and no copy of one; or what
// PSEvent.mapaligns makes of the lists (ps_remap.h): per pair a table part[i1] = i2 over seq1 (0 where the base faces a gap) that STAYS
// on the device, in a buffer of the caller's (SwJob::d_map), and a four-int record about it
enum SwForm { SW_LISTS = 0, SW_SUMMARY = 1, SW_MAP = 2 };

struct SwPair {
    int n1, n2;                  // rows (first sequence), columns (second sequence)
    int nrb;                     // row blocks of 64
    int ngw;                     // wave strips: waves x super-strips  (band: strips of SWBS columns)
    int pitch;                   // ints per saved row
    int wb;                      // band half-width (a multiple of 64; 0: the full matrix)
    int nbb;                     // band mode: row blocks of 64 kept per 512-column strip (8 + 2 wb / 64); full matrix: nrb
    int cpitch;                  // ints per saved column: n1 + 1, band mode 64 nbb + 1
    int64_t s1_off, s2_off;      // into the character pool
    int64_t row_off;             // rowsave: nrb x pitch ints, row q = H(64q, 1..n2) at [0..n2)  (band: strips x nbb x 512)
    int64_t col_off;             // colsave: (n2/64 + 1) x cpitch ints, entry c = H(0..n1, 64c)  (c = 0 unused)
    int64_t blk_off;             // blkmax: nrb x ngw ints  (band: strips x nbb)
    int64_t out_off;             // 2 * (n1 + n2 + 2) ints: index pairs in walk order; map form: n1 + 2 ints, the partner table part[i1] = i2
    int64_t res_off;             // SW_RES ints: the result record (SwRec)
};

// ---- the result record ----------------------------------------------------------------------------------------------------------
// summary form: the ends of the reversed index lists (entry 0, entry n_pairs - 1) and their zero entries; map form: RemapRec (ps_remap.h)
enum SwRec {
    SWR_SCORE = 0, SWR_BI = 1, SWR_BJ = 2, SWR_N_PAIRS = 3, SWR_N_MATCH = 4,
    SWR_TIMED_OUT = 5,   // a strip of the fill gave up waiting for its left neighbour
    SWR_INEXACT = 6,     // the band certificate failed
    SWR_FIRST1 = 8, SWR_FIRST2 = 9, SWR_LAST1 = 10, SWR_LAST2 = 11, SWR_GAP1 = 12, SWR_GAP2 = 13,
    SWR_MAP_LO = 8, SWR_MAP_HI = 9, SWR_MAP_HAS0 = 10, SWR_MAP_Y0 = 11,
};
PS_SW_HD inline int* sw_record(int* res, const SwPair& p) { return res + p.res_off; }               // a pair's record in the batch's pool ...
PS_SW_HD inline const int* sw_record(const int* res, const SwPair& p) { return res + p.res_off; }
PS_SW_HD inline int& sw_rec(int* record, SwRec f) { return record[f]; }                                // ... and one int of it
PS_SW_HD inline int sw_rec(const int* record, SwRec f) { return record[f]; }

// ---- addresses ------------------------------------------------------------------------------------------------------------------
// Every function has a form whose band / full decision is a template argument, for the fills (k_sw_fill is always full,
// k_sw_fill_pk<.., BAND> knows its mode), and the run-time form on p.wb that the traceback uses, which delegates to it.  A fill
// wave works on one strip s and computes its window once, w = band_win<BAND>(p, s): the compile-time forms take that window (the
// full forms ignore it; rs_index takes s, which it needs as well) where the run-time forms derive strip and window from the column.
PS_SW_HD inline int sw_min(int a, int b) { return a < b ? a : b; }
PS_SW_HD inline int sw_max(int a, int b) { return a > b ? a : b; }

// first row block kept by strip s (may be negative: the strip then starts at block 0); the strip's window, and that of the strip on its left
template <bool BAND> PS_SW_HD inline int band_lo(const SwPair& p, int s) { return BAND ? s * (SWBS / 64) - p.wb / 64 : 0; }
PS_SW_HD inline int band_lo(const SwPair& p, int s) { return p.wb ? band_lo<true>(p, s) : band_lo<false>(p, s); }
struct SwWin { int lo; };   // a strip's window of row blocks, by its first (a type of its own: not to be taken for a strip or a column)
template <bool BAND> PS_SW_HD inline SwWin band_win(const SwPair& p, int s) { return SwWin{band_lo<BAND>(p, s)}; }
template <bool BAND> PS_SW_HD inline SwWin band_left(SwWin w) { return SwWin{BAND ? w.lo - SWBS / 64 : 0}; }

// rowsave: H(64q, j + 1), the top boundary of row block q at 0-based column j of strip s
template <bool BAND> PS_SW_HD inline int64_t rs_index(const SwPair& p, int q, int j, int s) {
    return BAND ? p.row_off + ((int64_t)s * p.nbb + q - band_lo<true>(p, s)) * SWBS + (j - s * SWBS) : p.row_off + (int64_t)q * p.pitch + j;
}
PS_SW_HD inline int64_t rs_index(const SwPair& p, int q, int j) {
    if (!p.wb) return rs_index<false>(p, q, j, 0);
    return rs_index<true>(p, q, j, j / SWBS);
}

// colsave of column 64c, kept by the strip of window w, as a base index: entry i (H(i, 64c)) at [col_base + i] for
// rows 64 band_q0 <= i <= col_hi of that strip (outside: 0).  The compile-time form adds onto `base`: the pool's pointer in a fill
// (the uniform offset goes onto the pointer before the lane's column does), 0 for the plain index.
template <bool BAND, class B> PS_SW_HD inline B col_base(B base, const SwPair& p, int c, SwWin w) { return base + p.col_off + (int64_t)c * p.cpitch - (BAND ? 64 * w.lo : 0); }
PS_SW_HD inline int64_t col_base(const SwPair& p, int c) { return col_base<false>((int64_t)0, p, c, SwWin{0}) - (p.wb ? 64 * band_lo<true>(p, (64 * c - 1) / SWBS) : 0); }
template <bool BAND> PS_SW_HD inline int col_hi(const SwPair& p, SwWin w) { return BAND ? sw_min(p.n1, 64 * (w.lo + p.nbb)) : p.n1; }   // the strip's last row
PS_SW_HD inline int col_hi(const SwPair& p, int c) { return p.wb ? col_hi<true>(p, band_win<true>(p, (64 * c - 1) / SWBS)) : col_hi<false>(p, SwWin{0}); }

// blkmax of (row block q, wave strip gw)
template <bool BAND> PS_SW_HD inline int64_t bm_index(const SwPair& p, int q, int gw, SwWin w) {
    return BAND ? p.blk_off + (int64_t)gw * p.nbb + q - w.lo : p.blk_off + (int64_t)q * p.ngw + gw;
}
PS_SW_HD inline int64_t bm_index(const SwPair& p, int q, int gw) { return p.wb ? bm_index<true>(p, q, gw, band_win<true>(p, gw)) : bm_index<false>(p, q, gw, SwWin{0}); }
PS_SW_HD inline int64_t bm_base(const SwPair& p) { return p.blk_off; }   // the pair's maxima as one run: [bm_base, bm_base + bm_count)
PS_SW_HD inline int bm_count(const SwPair& p) { return (p.wb ? p.nbb : p.nrb) * p.ngw; }

// row blocks of a strip: the first, and one past the last
template <bool BAND> PS_SW_HD inline int band_q0(SwWin w) { return sw_max(0, BAND ? w.lo : 0); }
PS_SW_HD inline int band_q0(const SwPair& p, int gw) { return p.wb ? band_q0<true>(band_win<true>(p, gw)) : band_q0<false>(SwWin{0}); }
template <bool BAND> PS_SW_HD inline int band_q1(const SwPair& p, SwWin w) { return BAND ? sw_min(p.nrb, w.lo + p.nbb) : p.nrb; }
PS_SW_HD inline int band_q1(const SwPair& p, int gw) { return p.wb ? band_q1<true>(p, band_win<true>(p, gw)) : band_q1<false>(p, SwWin{0}); }

// the band certificate: a banded cell with Hb >= B(i, j) is exact, and a banded maximum above U = max B over all cells (reached
// out of band, at |i - j| = wb + 1) is the true one
PS_SW_HD inline int band_bound(int i, int j, int wb) { return 5 * sw_min(i, j) - 8 * sw_max(0, wb + 1 - abs(i - j)); }
PS_SW_HD inline int band_u(int n1, int n2, int wb) { return 5 * sw_max(0, sw_max(sw_min(n1, n2 - wb - 1), sw_min(n2, n1 - wb - 1))); }

// ---- placing a pair (host) --------------------------------------------------------------------------------------------------------
struct SwPools { int64_t row = 0, col = 0, blk = 0, out = 0, res = 0; };   // running totals of a batch's pools, in ints

// Pair p of lengths n1 x n2 in band mode wb (0: full matrix, filled with K columns per lane on WW waves per workgroup) behind what `t`
// already holds: everything of p but its characters' place.  (summary form: no index lists anywhere; map form: the table in the
// caller's buffer)
inline void sw_lay_out(SwPair& p, int n1, int n2, int wb, SwForm form, int K, int WW, SwPools& t) {
    p.n1 = n1; p.n2 = n2; p.wb = wb;
    p.nrb = sw_max(1, (n1 + 63) / 64);
    if (!wb) {
        const int sswidth = WW * 64 * K;
        p.ngw = WW * sw_max(1, (n2 + sswidth - 1) / sswidth);
        p.pitch = ((n2 + 3) / 4) * 4 + 4;
        p.nbb = p.nrb;
        p.cpitch = n1 + 1;
        p.row_off = t.row; t.row += (int64_t)p.nrb * p.pitch;
        p.blk_off = t.blk; t.blk += (int64_t)p.nrb * p.ngw;
    } else {
        p.ngw = sw_max(1, (n2 + SWBS - 1) / SWBS);
        p.pitch = SWBS;
        p.nbb = SWBS / 64 + 2 * wb / 64;
        p.cpitch = 64 * p.nbb + 1;
        p.row_off = t.row; t.row += (int64_t)p.ngw * p.nbb * SWBS;
        p.blk_off = t.blk; t.blk += (int64_t)p.ngw * p.nbb;
    }
    p.col_off = t.col; t.col += ((int64_t)n2 / 64 + 1) * p.cpitch;
    p.out_off = t.out; t.out += form == SW_LISTS ? 2 * ((int64_t)n1 + n2 + 2) : (form == SW_MAP ? (int64_t)n1 + 2 : 0);
    p.res_off = t.res; t.res += SW_RES;
}

// device order of a batch: the full-matrix pairs, then the band pairs (each group one fill and one traceback launch)
inline std::vector<int> sw_device_order(const std::vector<int>& wb) {
    std::vector<int> order;
    for (int pass = 0; pass < 2; pass++)
        for (int k = 0; k < (int)wb.size(); k++) if ((wb[k] != 0) == (pass == 1)) order.push_back(k);
    return order;
}

inline double band_cells(int n1, int n2, int wb) {   // cells the band fill computes
    const int nbb = SWBS / 64 + 2 * wb / 64, ns = (n2 + SWBS - 1) / SWBS, nrb = (n1 + 63) / 64;
    double c = 0;
    for (int s = 0; s < ns; s++) {
        const int lo = s * (SWBS / 64) - wb / 64, r0 = 64 * sw_max(0, lo), r1 = sw_min(n1, 64 * sw_min(nrb, lo + nbb));
        c += (double)sw_max(0, r1 - r0) * sw_min(SWBS, n2 - s * SWBS);
    }
    return c;
}

// Device bytes of one pair's checkpoints and (list form) index lists, as the chunking counts them (sw_chunk_end): an estimate beside
// sw_lay_out, not its sum.  It leaves out the block maxima, the result record and the rounding of pitch to whole fours (n2 + 8 stands
// for it), takes n1 / 64 and n2 / 64 as fractions, and in band mode counts a row block as 513 ints.  Its values decide where a
// batch is cut, so they stay as they are.  (map form: the pair's table lives in the caller's buffer, allocated for all pairs outside
// any chunking: nothing in a launch's pools)
inline double sw_pair_bytes(int n1, int n2, int wb, SwForm form = SW_LISTS) {
    const double out = form == SW_LISTS ? 8.0 * ((double)n1 + n2 + 2) : 0.0;
    if (!wb) return 4.0 * (((double)n1 / 64 + 1) * (n2 + 8) + ((double)n2 / 64 + 1) * (n1 + 1)) + out;
    const double nbb = SWBS / 64 + 2 * wb / 64, ns = (n2 + SWBS - 1) / SWBS;
    return 4.0 * (ns * nbb * (SWBS + 1) + ((double)n2 / 64 + 1) * (64 * nbb + 1)) + out;
}

}  // namespace ps
#endif
