// ps_edit.hip — gfx950 kernels of the edit scoring: ScoreMutations for every (event, edit) of a batch and what an edit-scoring
// call (ps_score.cpp) makes of that matrix.  They read the matrices, band tables and column maxima that the fills of
// ps_kernels.hip left behind, and share nothing with them but ps_dev.h.
//
// Reference behaviour being reproduced (file:line under the reference tree):
//   scoreMutation / columnMax     cpp/Alignment.cpp:447-512, cpp/Alignment.h:181-214
//   ScoreMutations accumulation   cpp/MakeMutations.cpp:23-69
//
//   k_old / k_oldall / k_oldfin   the score of the unedited sequence per distinct edit position
//   k_score / k_reduce            scoreMutation + columnMax per (event, edit), and the per-edit sums
//   k_point_table                 a point-table call: rows per position
//   k_support / k_genotype        a support / genotype call: scores, per-group records, likelihoods over the covering events
//   k_link / k_phase / k_haptag   a phase call's reductions of k_score's matrix: pair links, the scan over the sites, the reads' haplotypes
#include <algorithm>

#include "ps_internal.h"
#include "ps_dev.h"

namespace ps {

// ------------------------------------------------------------------------------------------------
// columnMax(raf, rab) on the filled matrices (cpp/Alignment.h:181-214); cooperative over `nl` lanes
// Only rows where both columns are in band can exceed the two running maxima (stay <= main <= max).
// ------------------------------------------------------------------------------------------------
// maximum over the NL lanes of a lane's group (groups of NL consecutive lanes from lane 0 of the wave on; wl: the lane in its wave).
// NL = 7 (nine groups to a wave, lane 63 idle): three rotations within the group — by 1, 2, 4: every lane then holds the maximum
// of 8 >= NL cyclically consecutive members.
template <int NL>
__device__ __forceinline__ double group_max(double v, int wl) {
    if ((NL & (NL - 1)) == 0) {
        for (int off = 1; off < NL; off <<= 1) v = fmax(v, __shfl_xor(v, off));
    } else {
        const int g0 = (wl / NL) * NL, c = wl - g0;
        for (int off = 1; off < NL; off <<= 1) v = fmax(v, __shfl(v, min(g0 + (c + off) % NL, 63)));
    }
    return v;
}

template <int NL>
__device__ double colmax_pair(const BatchD& b, const JobD& J, int raf, int rab, int lane, int wl) {
    constexpr int nl = NL;
    const int C = J.C, n0 = J.n0;
    if ((unsigned)raf >= (unsigned)(C + 1)) raf = C;
    if ((unsigned)rab >= (unsigned)(C + 1)) rab = C;
    const int* lb = b.lb + J.lb_off;
    int f0 = 0, f1 = n0, b0 = 0, b1 = n0;
    if (raf > 0) band_of(lb, 0, raf, C, n0, J.W, f0, f1);
    if (rab > 0) band_of(lb, 1, rab, C, n0, J.W, b0, b1);
    // jb = n0 - jf + 1 in [b0, b1]  <=>  jf in [n0 + 1 - b1, n0 + 1 - b0]
    const int lo = max(max(1, f0), n0 + 1 - b1), hi = min(min(n0, f1), n0 + 1 - b0);
    double sm = 0.0;
    for (int jf = lo + lane; jf <= hi; jf += nl) {
        const int jb = n0 - jf + 1;
        double2 fv = make_double2(0.0, 0.0), bv = make_double2(0.0, 0.0);
        if (raf > 0) fv = b.rec[rec_index(J, 0, jf, raf, f0)];
        if (rab > 0) bv = b.rec[rec_index(J, 1, jb, rab, b0)];
        sm = fmax(sm, fmax(fv.x + bv.x, fv.y + bv.y));
    }
    sm = group_max<NL>(sm, wl);
    sm = fmax(sm, b.pm[J.col_off[0] + raf]);
    sm = fmax(sm, b.pm[J.col_off[1] + rab]);
    return sm;
}

// old score for each distinct r0 = max(start - 3, 1) ; grid (nr0, njobs), block 64
__global__ __launch_bounds__(64) void k_old(BatchD b, const ScoreArgs* __restrict__ A) {
    const ScoreArgs& a = A[blockIdx.z];
    if (a.oldall || (int)blockIdx.x >= a.nr0 || (int)blockIdx.y >= a.njobs) return;
    const JobD& J = b.jobs[a.job0 + blockIdx.y];
    if (J.out->inert) return;
    const int r0 = a.r0[blockIdx.x];
    const double v = colmax_pair<64>(b, J, r0, J.C - r0 + 1, threadIdx.x, threadIdx.x);
    if (threadIdx.x == 0) a.old[(size_t)blockIdx.y * a.nr0 + blockIdx.x] = v;
}

// ------------------------------------------------------------------------------------------------
// columnMax(j, C - j + 1) for EVERY column j at once (the `old` score of all edit positions of a Refine / ScorePoints list).
// Cell (i, j) of the forward matrix lies on anti-diagonal s = i + j; its partner (n0 - i + 1, C - j + 1) of the backward matrix lies
// on anti-diagonal n0 + C + 2 - s, in the mirrored slot order: one pass over the anti-diagonals reads both matrices fully coalesced
// (32 B per cell), where one wave per column (k_old) touches a 128-byte line per 16-byte record.  Sums of two non-negative scores
// are maximised per column through an LDS window and one global atomic per touched column; max is order-independent, so the result
// is the reference's.  grid (ceil(S / OA_SB), njobs), block 256.
// ------------------------------------------------------------------------------------------------
constexpr int OA_SB = 32;      // anti-diagonals per block
constexpr int OA_COLS = 2048;  // column window of a block in LDS
__global__ __launch_bounds__(256) void k_oldall(BatchD b, const ScoreArgs* __restrict__ A) {
    __shared__ unsigned long long s_max[OA_COLS];
    __shared__ int s_jbase, s_ok;
    const ScoreArgs& a = A[blockIdx.z];
    if (!a.oldall || !a.nr0 || (int)blockIdx.y >= a.njobs) return;
    const JobD& J = b.jobs[a.job0 + blockIdx.y];
    if (J.out->inert || J.K) return;
    const int s0 = blockIdx.x * OA_SB;
    const int S = (int)J.S, P = J.P, n0 = J.n0, C = J.C;
    if (s0 >= S) return;
    const int nst = min(OA_SB, S - s0);
    const int* __restrict__ LOf = b.lo + J.lo_off[0];
    const int* __restrict__ HIf = b.hi + J.lo_off[0];
    const int* __restrict__ LOb = b.lo + J.lo_off[1];
    const int* __restrict__ HIb = b.hi + J.lo_off[1];
    if (threadIdx.x == 0) {
        int jmin = 0x7fffffff, jmax = -1;
        for (int k = 0; k < nst; k++) {
            const int lo = LOf[s0 + k];
            if (lo < 0) continue;
            jmax = max(jmax, s0 + k - lo);
            jmin = min(jmin, s0 + k - HIf[s0 + k]);
        }
        s_jbase = jmin;
        s_ok = jmax < 0 ? -1 : (jmax - jmin + 1 <= OA_COLS ? 1 : 0);
    }
    for (int k = threadIdx.x; k < OA_COLS; k += 256) s_max[k] = 0ull;
    __syncthreads();
    if (s_ok < 0) return;
    const bool use_lds = s_ok == 1;
    const int jbase = s_jbase;
    const double2* __restrict__ rf = b.rec + J.mat_off[0];
    const double2* __restrict__ rb = b.rec + J.mat_off[1];
    unsigned long long* gmax = (unsigned long long*)(a.oldall + (size_t)blockIdx.y * a.oldall_pitch);
    const int nP = P >> 6, lane = threadIdx.x & 63;
    int k = 0, c = threadIdx.x >> 6;
    while (c >= nP) { c -= nP; k++; }
    for (; k < nst;) {
        const int s = s0 + k;
        const int slot = c * 64 + lane;
        const int lo = __builtin_amdgcn_readfirstlane(LOf[s]), hi = __builtin_amdgcn_readfirstlane(HIf[s]);
        c += 4;
        while (c >= nP) { c -= nP; k++; }
        if (lo < 0) continue;
        int d = slot - lo % P;
        if (d < 0) d += P;
        const int i = lo + d;
        if (i > hi) continue;
        const int j = s - i;
        const int jb = n0 - i + 1, cb = C - j + 1, sb = jb + cb;      // partner cell in backward coordinates
        if (cb < 1) continue;                                           // (column j = C + 1 does not exist; cb = 0 is the blank column: sums with zero, covered by pm)
        const int lob = LOb[sb];
        if (lob < 0 || jb < lob || jb > HIb[sb]) continue;              // partner outside the backward band
        const double2 fv = rf[(int64_t)s * P + slot];
        const double2 bv = rb[(int64_t)sb * P + jb % P];
        const double v = fmax(fv.x + bv.x, fv.y + bv.y);
        if (v > 0.0) {
            const unsigned long long bits = (unsigned long long)__double_as_longlong(v);
            if (use_lds) atomicMax(&s_max[j - jbase], bits); else atomicMax(&gmax[j], bits);
        }
    }
    if (use_lds) {
        __syncthreads();
        for (int q = threadIdx.x; q < OA_COLS; q += 256) {
            const unsigned long long v = s_max[q];
            if (v) atomicMax(&gmax[jbase + q], v);
        }
    }
}

// The same pass over strip matrices (k_sweep2): the forward records of one step t and strip row r are NL consecutive records
// (one per lane = strip; NL = 64 per wavefront of a sweep); their partners in the backward matrix are 64 consecutive records too, in reverse order (row n0 - i + 1 of
// backward column C - j + 1: strip and step move by one per lane in opposite senses).  grid (ceil(maxT / OA_ST), njobs, regions), block 256.
constexpr int OA_ST = 16;      // steps per block
__global__ __launch_bounds__(256) void k_oldall_s(BatchD b, const ScoreArgs* __restrict__ A) {
    __shared__ unsigned long long s_max[OA_COLS];
    __shared__ int s_jbase, s_ok;
    const ScoreArgs& a = A[blockIdx.z];
    if (!a.oldall || !a.nr0 || (int)blockIdx.y >= a.njobs) return;
    const int job = a.job0 + blockIdx.y;
    const JobD& J = b.jobs[job];
    if (J.out->inert || !J.K) return;
    const SweepJob& SF = b.s_sj[2 * job];
    const SweepJob& SB = b.s_sj[2 * job + 1];
    const int K = J.K, T = SF.T, n0 = J.n0, C = J.C;
    const int t0 = blockIdx.x * OA_ST;
    if (t0 >= T) return;
    const int nst = min(OA_ST, T - t0);
    const int* __restrict__ QL = b.s_qlo + SF.q_off;
    const int* __restrict__ QH = b.s_qhi + SF.q_off;
    const int2* __restrict__ bandF = b.s_band + SF.band_off;
    const int2* __restrict__ bandB = b.s_band + SB.band_off;
    if (threadIdx.x == 0) {
        int jmin = 0x7fffffff, jmax = -1;
        for (int k = 0; k < nst; k++) {
            const int ql = QL[t0 + k];
            if (ql < 0) continue;
            jmax = max(jmax, t0 + k - ql);
            jmin = min(jmin, t0 + k - QH[t0 + k]);
        }
        s_jbase = jmin;
        s_ok = jmax < 0 ? -1 : (jmax - jmin + 1 <= OA_COLS ? 1 : 0);
    }
    for (int k = threadIdx.x; k < OA_COLS; k += 256) s_max[k] = 0ull;
    __syncthreads();
    if (s_ok < 0) return;
    const bool use_lds = s_ok == 1;
    const int jbase = s_jbase;
    const double2* __restrict__ rf = b.rec + J.mat_off[0];
    unsigned long long* gmax = (unsigned long long*)(a.oldall + (size_t)blockIdx.y * a.oldall_pitch);
    const int NL = J.NL, NWV = NL >> 6;                                  // lanes of a sweep, 64 per wavefront
    for (int p = threadIdx.x >> 6; p < nst * K * NWV; p += 4) {
        const int t = t0 + p / (K * NWV), r = (p / NWV) % K;
        const int lane = (p % NWV) * 64 + (threadIdx.x & 63);
        const int ql = __builtin_amdgcn_readfirstlane(QL[t]);
        if (ql < 0) continue;
        const int q = ql + ((lane - ql) & (NL - 1));
        const int i = q * K + 1 + r, j = t - q;
        if (j < 1 || j > C || i > n0) continue;
        const int2 bf = bandF[j];
        if (i < bf.x || i > bf.y) continue;
        const int ib = n0 - i + 1, cb = C - j + 1;                      // partner cell in backward coordinates
        const int2 bb = bandB[cb];
        if (ib < bb.x || ib > bb.y) continue;                           // partner outside the backward band
        const double2 fv = rf[((int64_t)t * K + r) * NL + lane];
        const double2 bv = b.rec[rec_index(J, 1, ib, cb, bb.x)];
        const double v = fmax(fv.x + bv.x, fv.y + bv.y);
        if (v > 0.0) {
            const unsigned long long bits = (unsigned long long)__double_as_longlong(v);
            if (use_lds) atomicMax(&s_max[j - jbase], bits); else atomicMax(&gmax[j], bits);
        }
    }
    if (use_lds) {
        __syncthreads();
        for (int q = threadIdx.x; q < OA_COLS; q += 256) {
            const unsigned long long v = s_max[q];
            if (v) atomicMax(&gmax[jbase + q], v);
        }
    }
}

// old[r0] = max(0, column sums, forward MaxInfo up to r0, backward MaxInfo up to C - r0 + 1)  (cpp/Alignment.h:181-214); grid (ceil(nr0/256), njobs)
__global__ __launch_bounds__(256) void k_oldfin(BatchD b, const ScoreArgs* __restrict__ A) {
    const ScoreArgs& a = A[blockIdx.z];
    if (!a.oldall || (int)blockIdx.y >= a.njobs) return;
    const JobD& J = b.jobs[a.job0 + blockIdx.y];
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= a.nr0 || J.out->inert) return;
    const int C = J.C;
    int raf = a.r0[q], rab = C - raf + 1;
    double sm = 0.0;
    if ((unsigned)raf >= (unsigned)(C + 1)) raf = C;           // columnMax's own clamping (cpp/Alignment.h:186-189)
    else sm = (a.oldall + (size_t)blockIdx.y * a.oldall_pitch)[raf];
    if ((unsigned)rab >= (unsigned)(C + 1)) rab = C;
    sm = fmax(sm, b.pm[J.col_off[0] + raf]);
    sm = fmax(sm, b.pm[J.col_off[1] + rab]);
    a.old[(size_t)blockIdx.y * a.nr0 + q] = sm;
}

// ------------------------------------------------------------------------------------------------
// scoreMutation (cpp/Alignment.cpp:447-512): G lanes per (event, edit) item, lane = new column,
// rows stream through the group systolically (lane c works on row  base + t - c  at step t).
// ------------------------------------------------------------------------------------------------
// (at most 96 VGPRs — five waves per SIMD: with 100 a workgroup's wave did not fit beside the two 208-register waves a lone k_fill
//  sweep keeps on SIMD 0 and 1, so k_score ran only on CUs without a fill: 1.07 ms per launch in the bench against 0.25 ms alone)
template <int G, bool FD>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5, 8))) void k_score(BatchD b, const ScoreArgs* __restrict__ A) {
    constexpr int IPW = 64 / G;   // (G = 7: nine items to a wave, lane 63 idle)
    constexpr int CLS = G == 7 ? 4 : G == 8 ? 0 : (G == 16 ? 1 : (G == 32 ? 2 : 3));
    const ScoreArgs& a = A[blockIdx.z];
    const int nitems = a.cls_count[CLS];
    if ((int)blockIdx.y >= a.njobs || (int)blockIdx.x * 4 * IPW >= nitems) return;
    const int* __restrict__ items = a.cls_items[CLS];
    __shared__ double s_carry[(G == 64) ? 4 * 1024 : 1];   // last column of a 64-column chunk, per wave
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane / G, c = lane % G;
    const int job = blockIdx.y;   // within the AlignData's own jobs, which start at a.job0 in the batch
    const JobD& J = b.jobs[a.job0 + job];
    const int it = (blockIdx.x * 4 + wave) * IPW + g;
    const bool have = it < nitems && g < IPW;
    const int m = have ? items[it] : 0;
    const int n0 = J.n0, C = J.C, WS = a.ws;
    const bool live = have && !J.out->inert && !a.m_skip[m];
    if (__ballot(live) == 0ull) {
        if (have && c == 0) a.delta[(size_t)job * a.nitems_per_job + m] = 0.0;
        return;
    }
    const int start = a.m_start[m], mlen = a.m_mlen[m], Cm = a.m_cm[m], ncol = live ? a.m_ncol[m] : 0;
    const int sidx = max(start - 4, 0);
    const int tcol = min(start + mlen + 1, sidx + ncol);   // target column (== sidx: the spliced copy itself)
    const int trel = tcol - sidx - 1;                      // 0-based new-column index of the target (-1: copy)
    int backind = Cm - tcol + 1;
    if ((unsigned)backind >= (unsigned)(C + 1)) backind = C;
    const int* __restrict__ lbf = b.lb + J.lb_off;    // tables the fills were made with
    const int* __restrict__ lbn = b.lb + J.lbn_off;   // after the backtrace: centres of the new columns
    // (the level records through a global-address-space pointer held in scalar registers: read through the job table the pointer is
    //  generic, and a FLAT load with 64-bit address arithmetic per row step costs nine vector instructions where this costs two)
    const PS_GLOBAL v4d* __restrict__ levf = (const PS_GLOBAL v4d*)uni_ptr(J.lev[0]);
    const double lsk = J.lsk, lst = J.lst, lex = J.lex, lin = J.lin;

    // band of the back column the target is combined with
    int bb0 = 0, bb1 = n0;
    if (backind > 0) band_of(lbf, 1, backind, C, n0, J.W, bb0, bb1);

    double fmaxv = live ? b.pm[J.col_off[0] + sidx] : 0.0;   // running MaxInfo score, carried from the spliced column
    double tm = 0.0;                                          // max over rows of fwd + back on the target column
    // previous column of the first chunk: the original forward column sidx (blank column 0 if sidx == 0)
    int pc0 = 0, pc1 = n0;
    if (live && sidx > 0) band_of(lbf, 0, sidx, C, n0, J.W, pc0, pc1);
    double* carry = s_carry + wave * 1024;

    const int nchunk = (ncol + G - 1) / G;
    int nchunk_w = nchunk;
    for (int off = 1; off < 64; off <<= 1) nchunk_w = max(nchunk_w, __shfl_xor(nchunk_w, off));
    for (int ch = 0; ch < nchunk_w; ch++) {
        const int cc = ch * G + c;                 // new-column index of this lane
        const bool mine = live && cc < ncol;
        const int jc = sidx + 1 + cc;              // column number in the edited sequence
        int i0 = 1, i1 = 0, state = -1;
        if (mine) {
            const int v = lbn[jc];
            const int ce = clampi(v < 0 ? 1 : v, 1, n0);
            i0 = max(1, ce - WS); i1 = min(n0, ce + WS);
            state = a.m_states[(size_t)m * a.ncolmax + cc];
        }
        // the column's model row as k_fill uses it: {mean, 1/stdv, stdv, log stdv, sd mean, 1/sd mean, lambda, log lambda}
        double mr[8] = {0, 1, 1, 0, 1, 1, 0, 0};
        if (state >= 0) {
            const double2* row = (const double2*)((const char*)J.model8 + (size_t)state * MODEL_ROW_BYTES);
            const double2 q0 = row[0], q1 = row[1], q2 = row[2], q3 = row[3];
            mr[0] = q0.x; mr[1] = q0.y; mr[2] = q1.x; mr[3] = q1.y; mr[4] = q2.x; mr[5] = q2.y; mr[6] = q3.x; mr[7] = q3.y;
        }
        // band of the column to the left
        int p0 = __shfl_up(i0, 1), p1 = __shfl_up(i1, 1);
        if (c == 0) { p0 = pc0; p1 = pc1; }
        const int base = __shfl(i0, g * G);                       // first row of the chunk's first column
        int lastcol = min(ncol - ch * G, G) - 1;                   // lanes 0..lastcol are in use
        int span = mine ? (i1 - base) + c : -1;
        for (int off = 1; off < 64; off <<= 1) span = max(span, __shfl_xor(span, off));
        double cm = 0.0, cs = 0.0, colmax = 0.0, lprev = 0.0;
        const bool is_t = mine && cc == trel;
        // The common case — skewed matrices, the item's columns in one chunk, no invalid 5-mer among them — runs a branch-free step:
        // every lane computes a cell on every step (on a clamped row outside its band) and what must not count is masked; the
        // matrix reads walk the skewed storage with cursors instead of index arithmetic per step.  Values are those of the general
        // loop below: candidates that are switched off there (no left / diagonal neighbour, top row) are -infinity, `lik_insert`
        // or `0 + x` here, which lose to the floors exactly where the reference's never-assigned candidates do.
        const bool use_f = mine && c == 0 && sidx > 0;          // lane 0 reads the spliced forward column
        const bool use_b = is_t && backind > 0;                  // the target lane reads the backward column
        // (a lane that reads both — an edit so close to the end of the sequence that its only new column is the target — takes the general loop)
        if (G < 64 && J.K <= 0 && __ballot((mine && state < 0) || (use_f && use_b)) == 0ull) {
            // (column-sparse records, J.K < 0: a column is one contiguous run of records, the cursors move by one; the wrap tests
            //  of the skewed storage never fire)
            const bool sp = J.K < 0;
            const int P = sp ? 0x40000000 : J.P;
            const unsigned stride = sp ? 1u : (unsigned)P + 1u;
            const double2* __restrict__ rf = b.rec + J.mat_off[0];
            const double2* __restrict__ rb = b.rec + J.mat_off[1];
            const double NINF = -__builtin_inf();
            int i = base - 1 - c;                                    // row of this lane on step t = -1
            int fslot = i >= 0 ? i % P : 0, bslot = (n0 - i + 1) % P;
            unsigned fidx = (unsigned)(max(i, 0) + sidx) * (unsigned)P + (unsigned)fslot;            // record of (i, sidx), forward matrix
            unsigned bidx = (unsigned)(n0 - i + 1 + backind) * (unsigned)P + (unsigned)bslot;        // record of (n0 - i + 1, backind), backward matrix
            if (sp) {
                fslot = 0; bslot = 0x7fffffff;
                fidx = use_f ? (unsigned)J.keep[0][sidx] * (unsigned)J.pitch + (unsigned)(i - pc0) : 0u;
                bidx = use_b ? (unsigned)J.keep[1][backind] * (unsigned)J.pitch + (unsigned)(n0 - i + 1 - bb0) : 0u;
            }
            // one cursor per lane: a lane reads the forward column (lane 0 of an item, `use_f`) or the backward one (the target lane,
            // `use_b`: new column len(mut) + 4 of the edit unless the sequence ends before) — not both (checked above)
            const bool bwd = use_b;
            unsigned idx = bwd ? bidx : fidx;
            int slot = bwd ? bslot : fslot;
            const int sgn = bwd ? -1 : 1, wrap_at = bwd ? 0 : P - 1, wrap_to = bwd ? P - 1 : 0;
            const unsigned dstride = bwd ? 0u - stride : stride;
            const double log2pi = b.log2pi, off = J.lik_offset;
            // forward level record of row i: {mean, stdv, 3 log stdv, 1 / stdv}; scalar base + unsigned 32-bit byte offset: one vector
            // instruction of address arithmetic.  (Fetched a step ahead it was 4 % slower, and the band masks as one high-word select
            // in front of a bare v_max_f64 9 % slower, than this loop: measured, `tools/gpu_scorebench.py`.)
            auto level_of = [&](int row) { return *(const PS_GLOBAL v4d*)((const PS_GLOBAL char*)levf + (unsigned)(32 * (clampi(row, 1, n0) - 1))); };
            for (int t = -1; t <= span; t++) {
                const v4d lv4 = level_of(i);
                double L = wave_shr1(cm);
                const bool vl = i >= p0 && i <= p1;
                if (c == 0) { L = 0.0; if (use_f && vl && i >= 1) L = rf[idx].x; }
                const double D = lprev;
                lprev = L;
                const bool inb = mine && i >= i0 && i <= i1;
                const double lev[4] = {lv4.x, lv4.y, lv4.z, lv4.w};
                const double o = emission8<FD>(mr, lev, log2pi, off);
                const bool vd = vl && i != p0, top = i == i0;
                const double Lz = vl ? L : 0.0, Dz = vd ? D : 0.0;
                const double um = top ? NINF : cm, us = top ? NINF : cs;
                const double cSKIP = Lz + lsk, cMATCH = Dz + o, cIGN = Dz + lin;
                const double cSTAY = um + o + lst, cEXT = us + o + lex, cINS = um + lin;
                const double ns = fmax(fmax(top ? -BIG : 0.0, cSTAY), cEXT);
                double nm = fmax(0.0, cSKIP);
                nm = fmax(nm, cMATCH);
                nm = fmax(nm, cINS);
                nm = fmax(nm, cIGN);
                nm = fmax(nm, ns);
                cm = nm; cs = ns;                                    // (rows outside the band leave garbage that nothing reads: the next in-band row is a top row)
                colmax = fmax(colmax, inb ? nm : 0.0);
                const int jb = n0 - i + 1;
                const bool hit = inb && is_t && jb >= bb0 && jb <= bb1;
                double2 bv = make_double2(0.0, 0.0);
                if (hit && use_b) bv = rb[idx];
                const double cand = fmax(nm + bv.x, ns + bv.y);
                tm = hit ? fmax(tm, cand) : tm;
                // next row: one anti-diagonal on, one slot on (forward); one back each (backward)
                i++;
                const bool wr = slot == wrap_at;
                idx += wr ? (unsigned)sgn : dstride; slot = wr ? wrap_to : slot + sgn;
            }
        } else {
            for (int t = -1; t <= span; t++) {
                const int i = base + t - c;
                // value of (i, jc-1): matrix / carried chunk column for lane 0, left neighbour otherwise
                double L = wave_shr1(cm);
                if (c == 0) {
                    L = 0.0;
                    if (mine && i >= p0 && i <= p1 && i >= 1) {
                        if (ch > 0) L = carry[i - p0];
                        else if (sidx > 0) L = b.rec[rec_index(J, 0, i, sidx, pc0)].x;
                    }
                }
                const double D = lprev;
                lprev = L;
                if (mine && i >= i0 && i <= i1) {
                    double nm = 0.0, ns = 0.0;
                    if (state >= 0) {
                        const v4d lv4 = levf[i - 1];       // forward level record of row i: {mean, stdv, 3 log stdv, 1 / stdv}
                        const double lev[4] = {lv4.x, lv4.y, lv4.z, lv4.w};
                        const double o = emission8<FD>(mr, lev, b.log2pi, J.lik_offset);
                        const bool vl = i >= p0 && i <= p1, vd = i > p0 && i <= p1;
                        const double cSKIP = vl ? L + lsk : lsk;
                        const double cMATCH = vd ? D + o : o;
                        const double cIGN = vd ? D + lin : 0.0;
                        double cSTAY = -BIG, cEXT = -BIG, cINS = 0.0;
                        if (i == i0) ns = -BIG;
                        else { cSTAY = cm + o + lst; cINS = cm + lin; cEXT = cs + o + lex; }
                        if (cSTAY > ns) ns = cSTAY;
                        if (cEXT > ns) ns = cEXT;
                        if (cSKIP > nm) nm = cSKIP;
                        if (cMATCH > nm) nm = cMATCH;
                        if (cINS > nm) nm = cINS;
                        if (cIGN > nm) nm = cIGN;
                        if (ns > nm) nm = ns;
                    }
                    cm = nm; cs = ns;
                    if (nm > colmax) colmax = nm;
                    if (is_t) {
                        const int jb = n0 - i + 1;
                        if (jb >= bb0 && jb <= bb1) {
                            double2 bv = make_double2(0.0, 0.0);
                            if (backind > 0) bv = b.rec[rec_index(J, 1, jb, backind, bb0)];
                            tm = fmax(tm, fmax(nm + bv.x, ns + bv.y));
                        }
                    }
                    if (G == 64 && c == lastcol && ch + 1 < nchunk) carry[i - i0] = nm;
                }
            }
        }
        // MaxInfo: max over the new columns up to and including the target
        double cmx = (mine && cc <= trel) ? colmax : 0.0;
        cmx = group_max<G>(cmx, lane);
        fmaxv = fmax(fmaxv, cmx);
        // next chunk continues from this chunk's last column
        pc0 = __shfl(i0, g * G + max(lastcol, 0)); pc1 = __shfl(i1, g * G + max(lastcol, 0));
        __builtin_amdgcn_wave_barrier();
    }
    // gather the target lane's row maximum
    const double tmx = group_max<G>(tm, lane);
    double now;
    if (trel < 0) {
        now = !live ? 0.0 : colmax_pair<G>(b, J, sidx, backind, c, lane);   // no new column: the spliced copy is the target
    } else {
        now = fmax(0.0, tmx);
        now = fmax(now, fmaxv);
        now = fmax(now, b.pm[J.col_off[1] + backind]);
    }
    if (have && c == 0) {
        double d = 0.0;
        if (live) {
            const double old = a.old[(size_t)job * a.nr0 + a.m_oldidx[m]];
            d = now - old;
        }
        a.delta[(size_t)job * a.nitems_per_job + m] = d;
    }
}

// score[m] = -1e-6 + sum over events in order (cpp/AlignUtil.h:86, cpp/MakeMutations.cpp:51)
__global__ void k_reduce(const ScoreArgs* __restrict__ A) {
    const ScoreArgs& a = A[blockIdx.y];
    const int njobs = a.njobs;
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= a.nitems_per_job) return;
    double s = -1e-6;
    for (int e = 0; e < njobs; e++) s += a.delta[(size_t)e * a.nitems_per_job + m];
    a.score[m] = s;
}

// k_reduce for FindPointMutations' list (cpp/FindMutations.cpp:200-228), laid out per position: table[p][9] = {deletion, substitution
// by A / C / G / T (a quiet NaN for the base itself, which the list does not hold), insertion of A / C / G / T}, and per position the
// largest entry, the first slot that holds it and the number of entries > 0 (ps_point_best, include/poreseq_hip.h).  A block owns
// PT_POS consecutive positions, i.e. one contiguous run of at most 9 PT_POS edits: a thread per edit adds the events' terms in event
// order (k_reduce's loop: plain FP64 adds, coalesced reads of delta[e][m]), then a thread per position lays its row out in LDS and
// the block writes the rows back to back.
constexpr int PT_POS = 28;   // 9 x 28 = 252 edits: one per thread of a 256-thread block
__global__ __launch_bounds__(256) void k_point_table(const ScoreArgs* __restrict__ A, const PointArgs* __restrict__ Q) {
    const ScoreArgs& a = A[blockIdx.y];
    const PointArgs& q = Q[blockIdx.y];
    const int p0 = blockIdx.x * PT_POS;
    if (p0 >= q.npos || !a.njobs) return;
    __shared__ double s_sum[PT_POS * PT_SLOTS], s_row[PT_POS * PT_SLOTS];
    const int np = min(PT_POS, q.npos - p0);
    const int m0 = q.pos_first[p0];
    const int nm = min(q.pos_first[p0 + np] - m0, PT_POS * PT_SLOTS);
    const int t = threadIdx.x;
    if (t < nm) {
        const int njobs = a.njobs;
        const int m = m0 + t;
        double s = -1e-6;
        for (int e = 0; e < njobs; e++) s += a.delta[(size_t)e * a.nitems_per_job + m];
        s_sum[t] = s;
    }
    __syncthreads();
    if (t < np) {
        const int p = p0 + t;
        const int at = q.pos_first[p] - m0, triv = q.pos_triv[p];
        double* row = s_row + PT_SLOTS * t;
        // (a list that is not FindPointMutations' would point past the block's run: such a row is all NaN instead of an LDS read out of bounds)
        const bool ok = at >= 0 && at + (triv ? 8 : 9) <= nm;
        int k = at;
        ps_point_best b;
        b.margin = -INFINITY; b.slot = 0; b.n_positive = 0;
        for (int sl = 0; sl < PT_SLOTS; sl++) {
            const double v = (!ok || (triv && sl == triv)) ? __builtin_nan("") : s_sum[k++];   // (triv == 0: every slot holds an edit)
            row[sl] = v;
            if (v > b.margin) { b.margin = v; b.slot = sl; }
            if (v > 0) b.n_positive++;
        }
        if (q.best) q.best[p] = b;
    }
    __syncthreads();
    if (q.table && t < PT_SLOTS * np) q.table[(size_t)PT_SLOTS * p0 + t] = s_row[t];
}

// k_reduce with the events' terms also added up per event group, and per (edit, group) the events that span the edit and how many
// of those have a positive / negative term (ps_edit_support, include/poreseq_hip.h).  A thread per edit walks the events in order
// (k_reduce's coalesced reads of delta[e][m], plain FP64 adds).  An event's group id and its re-aligned span (JobOut.has_index /
// refstart / refend as k_updaterefs left them behind the backtrace) are the same for every thread of a step: the block stages them
// in LDS, SUP_EV events at a time.  The accumulators are never indexed by a runtime value (they would go to scratch): the loop over
// g is unrolled over all SUPPORT_MAX_GROUPS and `acc[g] += (grp == g) ? d : 0.0` leaves the other groups' sums as they are — an
// accumulator starts at +0.0 and can therefore never be -0.0, the one value that adding +0.0 would change.
constexpr int SUP_EV = 256;
__global__ __launch_bounds__(256) void k_support(BatchD b, const ScoreArgs* __restrict__ A, const SupportArgs* __restrict__ Q) {
    const ScoreArgs& a = A[blockIdx.y];
    const SupportArgs& q = Q[blockIdx.y];
    const int M = a.nitems_per_job, njobs = a.njobs, G = q.ngroups;
    if ((int)(blockIdx.x * blockDim.x) >= M || !njobs || !G) return;   // (the same for every thread of the block)
    __shared__ int s_grp[SUP_EV], s_lo[SUP_EV], s_hi[SUP_EV];
    const int t = threadIdx.x;
    const int m = blockIdx.x * blockDim.x + t;
    const bool have = m < M;
    // column of the 5-mer that begins at the edit's first base; a skipped edit (start > length) is spanned by no event
    const int col = (have && !a.m_skip[m]) ? a.m_start[m] + 1 : -0x7fffffff;
    double s = -1e-6;
    double acc[SUPPORT_MAX_GROUPS];
    int cov[SUPPORT_MAX_GROUPS], pos[SUPPORT_MAX_GROUPS], neg[SUPPORT_MAX_GROUPS];
#pragma unroll
    for (int g = 0; g < SUPPORT_MAX_GROUPS; g++) { acc[g] = 0.0; cov[g] = 0; pos[g] = 0; neg[g] = 0; }
    for (int e0 = 0; e0 < njobs; e0 += SUP_EV) {
        if (e0) __syncthreads();   // (everyone is done with the previous events)
        if (e0 + t < njobs) {
            const JobOut* O = b.jobs[a.job0 + e0 + t].out;
            const bool span = O->has_index != 0;     // a positive ref_align entry: refstart / refend are the int of the first / last
            s_grp[t] = q.group[e0 + t];
            s_lo[t] = span ? O->refstart : 1;
            s_hi[t] = span ? O->refend : 0;
        }
        __syncthreads();
        const int ne = min(SUP_EV, njobs - e0);
        if (have)
            for (int k = 0; k < ne; k++) {
                const double d = a.delta[(size_t)(e0 + k) * M + m];
                s += d;
                const int grp = s_grp[k];
                const bool cv = s_lo[k] <= col && col <= s_hi[k];
#pragma unroll
                for (int g = 0; g < SUPPORT_MAX_GROUPS; g++) {
                    const bool in = grp == g;
                    acc[g] += in ? d : 0.0;
                    cov[g] += (in && cv) ? 1 : 0;
                    pos[g] += (in && cv && d > 0) ? 1 : 0;
                    neg[g] += (in && cv && d < 0) ? 1 : 0;
                }
            }
    }
    if (!have) return;
    q.score[m] = s;
#pragma unroll
    for (int g = 0; g < SUPPORT_MAX_GROUPS; g++)
        if (g < G) {
            ps_edit_support r;
            r.sum = acc[g]; r.cover = cov[g]; r.pos = pos[g]; r.neg = neg[g]; r.reserved = 0;
            q.out[(size_t)m * G + g] = r;
        }
}

// Genotype likelihoods per edit (ps_score_mutation_genotypes, include/poreseq_hip.h): a second reduction of the delta matrix that
// k_support has just read, over the events that SPAN the edit only (k_support's `cv`).  For an alt fraction f with g = 1 - f a
// covering event adds log(g + f e^d), evaluated as max(d, 0) + log(x) with u = exp(-|d|) and x = g u + f (d > 0) or g + f u: one
// exp per (event, edit) and one log per fraction, no positive exponent, x in [min(f, g), 1].  The hom-alt column is the covering
// events' terms in plain FP64 adds.  k_support's shape: a thread per edit, events in order, coalesced reads of delta[e][m], the
// events' spans staged in LDS SUP_EV at a time behind the same two barriers.  The accumulators are never indexed by a runtime
// value: the loop over k is unrolled over all GENO_MAX_FRAC and `k < K` (the same for the whole block) guards each.
__global__ __launch_bounds__(256) void k_genotype(BatchD b, const ScoreArgs* __restrict__ A, const GenoArgs* __restrict__ Q) {
    const ScoreArgs& a = A[blockIdx.y];
    const GenoArgs& q = Q[blockIdx.y];
    const int M = a.nitems_per_job, njobs = a.njobs, K = q.nfrac;
    if ((int)(blockIdx.x * blockDim.x) >= M || !njobs || K < 0) return;   // (the same for every thread of the block)
    __shared__ int s_lo[SUP_EV], s_hi[SUP_EV];
    const int t = threadIdx.x;
    const int m = blockIdx.x * blockDim.x + t;
    const bool have = m < M;
    // column of the 5-mer that begins at the edit's first base; a skipped edit (start > length) is spanned by no event
    const int col = (have && !a.m_skip[m]) ? a.m_start[m] + 1 : -0x7fffffff;
    double s = -1e-6, hom = 0.0;
    int nc = 0;
    double acc[GENO_MAX_FRAC];
#pragma unroll
    for (int k = 0; k < GENO_MAX_FRAC; k++) acc[k] = 0.0;
    for (int e0 = 0; e0 < njobs; e0 += SUP_EV) {
        if (e0) __syncthreads();   // (everyone is done with the previous events)
        if (e0 + t < njobs) {
            const JobOut* O = b.jobs[a.job0 + e0 + t].out;
            const bool span = O->has_index != 0;
            s_lo[t] = span ? O->refstart : 1;
            s_hi[t] = span ? O->refend : 0;
        }
        __syncthreads();
        const int ne = min(SUP_EV, njobs - e0);
        if (have)
            for (int i = 0; i < ne; i++) {
                const double d = a.delta[(size_t)(e0 + i) * M + m];
                s += d;
                if (s_lo[i] <= col && col <= s_hi[i]) {
                    nc++;
                    hom += d;
                    const bool up = d > 0;
                    const double u = exp(-fabs(d)), top = up ? d : 0.0;
#pragma unroll
                    for (int k = 0; k < GENO_MAX_FRAC; k++)
                        if (k < K) {
                            const double x = up ? q.g[k] * u + q.f[k] : q.g[k] + q.f[k] * u;
                            acc[k] += top + log(x);
                        }
                }
            }
    }
    if (!have) return;
    if (q.score) q.score[m] = s;
    q.ncover[m] = nc;
    double* out = q.lik + (size_t)m * (K + 1);
#pragma unroll
    for (int k = 0; k < GENO_MAX_FRAC; k++)
        if (k < K) out[k] = acc[k];
    out[K] = hom;
}

// Pair links of a phase call (ps_score_mutation_phase, include/poreseq_hip.h): per edit m and w = 1 .. W the pair (m, m + w) over
// the events that span both, as the likelihood of both alts on one chromosome copy (cis) and of one on each (trans).
// k_genotype's shape: a thread per edit, events in order, coalesced reads of delta[e][m], the events' spans staged in LDS SUP_EV at
// a time.  The partner terms delta[e][m + w] come from the same row (lane t reads the word w further on: the same lines, and for
// the last threads of a block the lines of the next block's range).  The accumulators are never indexed by a runtime value: the
// loop over w is unrolled over all LINK_MAX_WINDOW, `w <= W` (the same for the whole block) guards each, and the partner's column
// is -0x7fffffff — spanned by no event — where m + w >= M or the partner is skipped.
__global__ __launch_bounds__(256) void k_link(BatchD b, const ScoreArgs* __restrict__ A, const PhaseArgs* __restrict__ Q) {
    const ScoreArgs& a = A[blockIdx.y];
    const PhaseArgs& q = Q[blockIdx.y];
    const int M = a.nitems_per_job, njobs = a.njobs, W = q.W;
    if ((int)(blockIdx.x * blockDim.x) >= M || !njobs || !W) return;   // (the same for every thread of the block)
    __shared__ int s_lo[SUP_EV], s_hi[SUP_EV];
    const int t = threadIdx.x;
    const int m = blockIdx.x * blockDim.x + t;
    const bool have = m < M;
    const int none = -0x7fffffff;
    const int col = (have && !a.m_skip[m]) ? a.m_start[m] + 1 : none;
    int colw[LINK_MAX_WINDOW], nb[LINK_MAX_WINDOW], ncis[LINK_MAX_WINDOW], ntr[LINK_MAX_WINDOW];
    double cis[LINK_MAX_WINDOW], trans[LINK_MAX_WINDOW];
#pragma unroll
    for (int w = 0; w < LINK_MAX_WINDOW; w++) {
        const int j = m + w + 1;
        colw[w] = (w < W && j < M && !a.m_skip[j]) ? a.m_start[j] + 1 : none;
        cis[w] = 0.0; trans[w] = 0.0; nb[w] = 0; ncis[w] = 0; ntr[w] = 0;
    }
    double s = -1e-6;
    for (int e0 = 0; e0 < njobs; e0 += SUP_EV) {
        if (e0) __syncthreads();   // (everyone is done with the previous events)
        if (e0 + t < njobs) {
            const JobOut* O = b.jobs[a.job0 + e0 + t].out;
            const bool span = O->has_index != 0;
            s_lo[t] = span ? O->refstart : 1;
            s_hi[t] = span ? O->refend : 0;
        }
        __syncthreads();
        const int ne = min(SUP_EV, njobs - e0);
        if (have)
            for (int i = 0; i < ne; i++) {
                const double* row = a.delta + (size_t)(e0 + i) * M;
                const double da = row[m];
                s += da;
                const int lo = s_lo[i], hi = s_hi[i];
                if (lo <= col && col <= hi) {
#pragma unroll
                    for (int w = 0; w < LINK_MAX_WINDOW; w++)
                        if (lo <= colw[w] && colw[w] <= hi) {   // (never true past W or past the list's end)
                            const double db = row[m + w + 1];
                            const double sm = da + db, r = da - db;
                            cis[w] += (sm > 0 ? sm : 0.0) + log(0.5 + 0.5 * exp(-fabs(sm)));
                            trans[w] += (da > db ? da : db) + log(0.5 + 0.5 * exp(-fabs(r)));
                            nb[w]++;
                            ncis[w] += ((da > 0 && db > 0) || (da < 0 && db < 0)) ? 1 : 0;
                            ntr[w] += ((da > 0 && db < 0) || (da < 0 && db > 0)) ? 1 : 0;
                        }
                }
            }
    }
    if (!have) return;
    if (q.score) q.score[m] = s;
#pragma unroll
    for (int w = 0; w < LINK_MAX_WINDOW; w++)
        if (w < W) {
            ps_edit_link r;
            r.cis = cis[w]; r.trans = trans[w]; r.n_both = nb[w]; r.n_cis = ncis[w]; r.n_trans = ntr[w]; r.reserved = 0;
            q.link[(size_t)m * W + w] = r;
        }
}

// The phase scan of a phase call: one wavefront per AlignData walks the sites in list order, PH_CHUNK at a time, a lane per site.
// The link records the chunk's sites look back at — those of the sites c0 - LINK_MAX_WINDOW .. c0 + PH_CHUNK - 1, contiguous in
// memory — are read by all lanes side by side and left in LDS as cis - trans and n_both > 0, and every lane takes its own site's W
// differences into registers: everything that does not depend on the chain is done before it starts.  The chain itself is the
// sign only: in step l every lane forms "its vote, were it site l's turn" from its differences and the wave-uniform history (the
// last LINK_MAX_WINDOW haplotype signs, and `run`, the number of sites ending at m - 1 that share its set: phase[m - w].set ==
// phase[m - 1].set is w <= run), lane l's decision is read with one v_readlane, and the history moves on.  A lane keeps the vote,
// haplotype and set of its own step and the chunk's records go out side by side.  Nothing of the chain goes through memory.
// WM is the largest window of the launch's AlignData, rounded up to 1, 2, 4 or 8: a step costs WM multiply-adds, and the history's
// update is written as selects, not branches.
constexpr int PH_CHUNK = 64;
template <int WM> __global__ __launch_bounds__(64) void k_phase(const ScoreArgs* __restrict__ A, const PhaseArgs* __restrict__ Q) {
    const ScoreArgs& a = A[blockIdx.x];
    const PhaseArgs& q = Q[blockIdx.x];
    const int M = a.nitems_per_job, W = q.W;
    if (!M || !a.njobs || !W) return;
    __shared__ double s_diff[(PH_CHUNK + LINK_MAX_WINDOW) * LINK_MAX_WINDOW];
    __shared__ int s_ok[(PH_CHUNK + LINK_MAX_WINDOW) * LINK_MAX_WINDOW];
    const int t = threadIdx.x;
    const double min_link = q.min_link;
    double h[WM];   // hap of site m - 1 .. m - WM (wave-uniform; only ever indexed by unrolled loops)
#pragma unroll
    for (int w = 0; w < WM; w++) h[w] = 1.0;
    int run = 0, set = 0;
    for (int c0 = 0; c0 < M; c0 += PH_CHUNK) {
        const int n = min(PH_CHUNK, M - c0);
        const int b0 = c0 - LINK_MAX_WINDOW;   // the first site whose records are staged (negative in the first chunk: none before site 0)
        if (c0) __syncthreads();               // (everyone has taken its differences of the previous chunk)
        for (int r = t; r < (n + LINK_MAX_WINDOW) * W; r += 64) {
            const int site = b0 + r / W;
            if (site < 0) continue;
            const ps_edit_link L = q.link[(int64_t)b0 * W + r];
            s_diff[r] = L.cis - L.trans;
            s_ok[r] = L.n_both > 0;
        }
        __syncthreads();
        const int m = c0 + t;
        double dv[WM];
        int okm = 0;   // bit w - 1: the pair (m - w, m) exists and has shared events
#pragma unroll
        for (int w = 1; w <= WM; w++) {
            const bool use = t < n && w <= W && w <= m;
            const int r = (t + LINK_MAX_WINDOW - w) * W + (w - 1);   // record w - 1 of site m - w
            dv[w - 1] = use ? s_diff[use ? r : 0] : 0.0;
            if (use && s_ok[r]) okm |= 1 << (w - 1);
        }
        double myvote = 0.0;
        int myhap = 1, myset = 0;
        for (int l = 0; l < n; l++) {
            double vote = 0.0;
#pragma unroll
            for (int w = 1; w <= WM; w++)
                if (((okm >> (w - 1)) & 1) && w <= run) vote += h[w - 1] * dv[w - 1];
            int code = (vote != 0.0 && fabs(vote) >= min_link) ? (vote > 0 ? 1 : -1) : 0;   // (a NaN fails both)
            if (c0 + l == 0) code = 2;   // site 0 opens set 0
            const int c = __builtin_amdgcn_readlane(code, l);
            const bool first = c == 2, join = c == 1 || c == -1;
            const int hap = join ? c : 1;
            run = join ? run + 1 : 1;
            set = first ? 0 : (join ? set : set + 1);
            if (t == l) { myvote = vote; myhap = hap; myset = set; }
#pragma unroll
            for (int w = WM - 1; w > 0; w--) h[w] = h[w - 1];
            h[0] = (double)hap;
        }
        if (t < n) {
            ps_edit_phase p;
            p.vote = myvote; p.hap = myhap; p.set = myset;
            q.phase[c0 + t] = p;
        }
    }
    if (t == 0) *q.nsets = set + 1;
}

// Read haplotypes of a phase call: one wavefront per event adds the event's terms over the sites of every tagged phase set, by the
// site's haplotype.  Lane l walks the sites l, l + 64, ... ascending (coalesced reads of delta[e][m] and of the phase records) into
// partials of its own, and the 64 partials of a sum are then added in lane order by one thread: an order a host can reproduce.
// As in k_support the accumulators are never indexed by a runtime value: the loop over the sets is unrolled over all
// PHASE_MAX_SETS and a site adds +0.0 to the sums it does not belong to, which leaves them as they are (a sum that starts at +0.0
// is never -0.0).
__global__ __launch_bounds__(64) void k_haptag(BatchD b, const ScoreArgs* __restrict__ A, const PhaseArgs* __restrict__ Q) {
    const ScoreArgs& a = A[blockIdx.y];
    const PhaseArgs& q = Q[blockIdx.y];
    const int M = a.nitems_per_job, njobs = a.njobs, S = q.S, e = blockIdx.x;
    if (e >= njobs || !M || !q.W || !q.hap) return;   // (the same for every thread of the block)
    __shared__ double s_sum[2 * PHASE_MAX_SETS][64];
    __shared__ int s_cnt[2 * PHASE_MAX_SETS][64];
    const int t = threadIdx.x;
    const JobOut* O = b.jobs[a.job0 + e].out;
    const bool span = O->has_index != 0;
    const int lo = span ? O->refstart : 1, hi = span ? O->refend : 0;
    double l1[PHASE_MAX_SETS], l2[PHASE_MAX_SETS];
    int n1[PHASE_MAX_SETS], n2[PHASE_MAX_SETS];
#pragma unroll
    for (int k = 0; k < PHASE_MAX_SETS; k++) { l1[k] = 0.0; l2[k] = 0.0; n1[k] = 0; n2[k] = 0; }
    const double* row = a.delta + (size_t)e * M;
    for (int m = t; m < M; m += 64) {
        const int col = a.m_skip[m] ? -0x7fffffff : a.m_start[m] + 1;
        if (!(lo <= col && col <= hi)) continue;
        const double d = row[m];
        const ps_edit_phase p = q.phase[m];
#pragma unroll
        for (int k = 0; k < PHASE_MAX_SETS; k++) {
            const bool one = p.set == k && p.hap > 0, two = p.set == k && p.hap < 0;
            l1[k] += one ? d : 0.0; n1[k] += one ? 1 : 0;
            l2[k] += two ? d : 0.0; n2[k] += two ? 1 : 0;
        }
    }
#pragma unroll
    for (int k = 0; k < PHASE_MAX_SETS; k++) {
        s_sum[2 * k][t] = l1[k]; s_sum[2 * k + 1][t] = l2[k];
        s_cnt[2 * k][t] = n1[k]; s_cnt[2 * k + 1][t] = n2[k];
    }
    __syncthreads();
    if (t < 2 * S) {   // thread 2 k: lik1 / n1 of set k; thread 2 k + 1: lik2 / n2
        double sum = 0.0;
        int cnt = 0;
        for (int l = 0; l < 64; l++) { sum += s_sum[t][l]; cnt += s_cnt[t][l]; }
        ps_event_hap* out = q.hap + (size_t)e * S + (t >> 1);
        if (t & 1) { out->lik2 = sum; out->n2 = cnt; }
        else { out->lik1 = sum; out->n1 = cnt; }
    }
}

// the tails of launch_score: what is made of the [event][edit] matrix k_score left behind
// a point-table call (every AlignData of it): rows per position instead of a score per edit
static int launch_point_table(Runtime* rt, const ScoreLaunch& L) {
    const int R = (int)L.sas.size();
    int maxnpos = 0;
    double bytes = 0;
    for (int k = 0; k < R; k++) {
        const ScoreArgs& a = L.sas[k];
        const int npos = L.pts[k].npos;
        if (!a.njobs || !npos) continue;
        maxnpos = std::max(maxnpos, npos);
        bytes += 8.0 * a.njobs * a.nitems_per_job + 88.0 * npos;
    }
    if (!maxnpos) return PS_OK;
    prof_begin(rt);
    hipLaunchKernelGGL(k_point_table, dim3((maxnpos + PT_POS - 1) / PT_POS, R), dim3(256), 0, rt->stream, L.d_sas, L.d_pts);
    PS_LAUNCH_CHECK();
    prof_end(rt, "point_table", bytes);
    return PS_OK;
}

// a support call (every AlignData of it): the score per edit and a record per (edit, group)
static int launch_support(Runtime* rt, const BatchD& b, const ScoreLaunch& L, int maxM) {
    const int R = (int)L.sas.size();
    double bytes = 0;
    // (a genotype call may want no support records anywhere: k_support then has nothing to write; a support call always launches it)
    bool any_records = L.kind != EditKind::Genotype;
    for (int k = 0; k < R; k++) {
        const ScoreArgs& a = L.sas[k];
        if (!a.njobs || !a.nitems_per_job || !L.sps[k].ngroups) continue;
        any_records = true;
        bytes += 8.0 * a.njobs * a.nitems_per_job + (8.0 + 24.0 * L.sps[k].ngroups) * a.nitems_per_job;
    }
    if (!any_records) return PS_OK;
    prof_begin(rt);
    hipLaunchKernelGGL(k_support, dim3((maxM + 255) / 256, R), dim3(256), 0, rt->stream, b, L.d_sas, L.d_sps);
    PS_LAUNCH_CHECK();
    prof_end(rt, "support", bytes);
    return PS_OK;
}

// a genotype call, behind launch_support: the same matrix reduced once more, over the covering events
static int launch_genotype(Runtime* rt, const BatchD& b, const ScoreLaunch& L, int maxM) {
    const int R = (int)L.sas.size();
    double bytes = 0;
    for (int k = 0; k < R; k++) {
        const ScoreArgs& a = L.sas[k];
        if (!a.njobs || !a.nitems_per_job || L.gts[k].nfrac < 0) continue;
        bytes += 8.0 * a.njobs * a.nitems_per_job + (8.0 * (L.gts[k].nfrac + 1) + 4.0) * a.nitems_per_job;
    }
    prof_begin(rt);
    hipLaunchKernelGGL(k_genotype, dim3((maxM + 255) / 256, R), dim3(256), 0, rt->stream, b, L.d_sas, L.d_gts);
    PS_LAUNCH_CHECK();
    prof_end(rt, "genotype", bytes);
    return PS_OK;
}

// a phase call (every AlignData of it): the score and the pair links per edit, the scan over the sites, the records per event
static int launch_phase(Runtime* rt, const BatchD& b, const ScoreLaunch& L, int maxM, int maxE) {
    const int R = (int)L.sas.size();
    double link_bytes = 0, phase_bytes = 0, tag_bytes = 0;
    bool any = false, any_hap = false;
    int maxW = 0;
    for (int k = 0; k < R; k++) {
        const ScoreArgs& a = L.sas[k];
        const PhaseArgs& q = L.phs[k];
        if (!a.njobs || !a.nitems_per_job || !q.W) continue;
        any = true;
        maxW = std::max(maxW, q.W);
        link_bytes += 8.0 * a.njobs * a.nitems_per_job + 32.0 * q.W * a.nitems_per_job;
        phase_bytes += (32.0 * q.W + 16.0) * a.nitems_per_job;
        if (!q.hap) continue;
        any_hap = true;
        tag_bytes += 8.0 * a.njobs * a.nitems_per_job + 16.0 * a.nitems_per_job + 24.0 * q.S * a.njobs;
    }
    if (!any) return PS_OK;
    prof_begin(rt);
    hipLaunchKernelGGL(k_link, dim3((maxM + 255) / 256, R), dim3(256), 0, rt->stream, b, L.d_sas, L.d_phs);
    PS_LAUNCH_CHECK();
    prof_end(rt, "link", link_bytes);
    prof_begin(rt);
    if (maxW <= 1) hipLaunchKernelGGL(k_phase<1>, dim3(R), dim3(64), 0, rt->stream, L.d_sas, L.d_phs);
    else if (maxW <= 2) hipLaunchKernelGGL(k_phase<2>, dim3(R), dim3(64), 0, rt->stream, L.d_sas, L.d_phs);
    else if (maxW <= 4) hipLaunchKernelGGL(k_phase<4>, dim3(R), dim3(64), 0, rt->stream, L.d_sas, L.d_phs);
    else hipLaunchKernelGGL(k_phase<8>, dim3(R), dim3(64), 0, rt->stream, L.d_sas, L.d_phs);
    PS_LAUNCH_CHECK();
    prof_end(rt, "phase", phase_bytes);
    if (!any_hap) return PS_OK;   // (no caller wants the events tagged)
    prof_begin(rt);
    hipLaunchKernelGGL(k_haptag, dim3(maxE, R), dim3(64), 0, rt->stream, b, L.d_sas, L.d_phs);
    PS_LAUNCH_CHECK();
    prof_end(rt, "haptag", tag_bytes);
    return PS_OK;
}

// edit scoring of several AlignData of one batch (L: their descriptors on the host and on the device): one launch per kernel over
// all of them — grid.z (k_reduce: grid.y) is the AlignData, blocks past an AlignData's own sizes leave at once
int launch_score(Runtime* rt, const BatchD& b, const ScoreLaunch& L) {
    const ScoreArgs* d_sas = L.d_sas;
    const int R = (int)L.sas.size();
    int maxE = 0, maxnr0 = 0, maxnr0_all = 0, maxM = 0, cls_max[SCORE_CLASSES] = {0, 0, 0, 0, 0};
    int64_t maxS = 0;
    bool any_all = false, any_old = false;
    for (const ScoreArgs& a : L.sas) {
        if (!a.njobs || !a.nitems_per_job) continue;
        maxE = std::max(maxE, a.njobs); maxM = std::max(maxM, a.nitems_per_job);
        if (a.nr0 > 0 && a.oldall) { any_all = true; maxS = std::max(maxS, a.maxS); maxnr0_all = std::max(maxnr0_all, a.nr0); }
        else if (a.nr0 > 0) { any_old = true; maxnr0 = std::max(maxnr0, a.nr0); }
        for (int k = 0; k < SCORE_CLASSES; k++) cls_max[k] = std::max(cls_max[k], a.cls_count[k]);
    }
    if (!maxE || !maxM) return PS_OK;
    if (any_all) {
        // a list that touches most columns (Refine, ScorePoints): one coalesced pass over both matrices serves every position
        // (the caller has zeroed the oldall arrays)
        if (b.s_sj) hipLaunchKernelGGL(k_oldall_s, dim3((unsigned)((maxS + OA_ST - 1) / OA_ST), maxE, R), dim3(256), 0, rt->stream, b, d_sas);   // (maxS >= every T)
        else hipLaunchKernelGGL(k_oldall, dim3((unsigned)((maxS + OA_SB - 1) / OA_SB), maxE, R), dim3(256), 0, rt->stream, b, d_sas);
        hipLaunchKernelGGL(k_oldfin, dim3((maxnr0_all + 255) / 256, maxE, R), dim3(256), 0, rt->stream, b, d_sas);
        PS_LAUNCH_CHECK();
    }
    if (any_old) {
        hipLaunchKernelGGL(k_old, dim3(maxnr0, maxE, R), dim3(64), 0, rt->stream, b, d_sas);
        PS_LAUNCH_CHECK();
    }
    prof_begin(rt);
    for (int k = 0; k < SCORE_CLASSES; k++) {
        const int n = cls_max[k];
        if (!n) continue;
        const int G = score_class_lanes(k), ipb = 4 * (64 / G);
        dim3 grid((n + ipb - 1) / ipb, maxE, R), block(256);
#define PS_SCORE(GG) with_fastdiv(b.fastdiv, [&](auto fd) { hipLaunchKernelGGL((k_score<GG, fd.value>), grid, block, 0, rt->stream, b, d_sas); })
        if (G == 7) PS_SCORE(7); else if (G == 8) PS_SCORE(8); else if (G == 16) PS_SCORE(16); else if (G == 32) PS_SCORE(32); else PS_SCORE(64);
#undef PS_SCORE
        PS_LAUNCH_CHECK();
        if (rt->prof_on) {   // (which size class ran, and whether it divided: host-side counts)
            static const char* const cls_name[SCORE_CLASSES] = {"score_g8", "score_g16", "score_g32", "score_g64", "score_g7"};
            rt->prof[cls_name[k]].launches++;
            if (!b.fastdiv) rt->prof["score_ieee"].launches++;
        }
    }
    prof_end(rt, "score", 0.0);
    switch (L.kind) {
    case EditKind::Points: return launch_point_table(rt, L);
    case EditKind::Genotype: PS_TRY(launch_support(rt, b, L, maxM)); return launch_genotype(rt, b, L, maxM);
    case EditKind::Support: return launch_support(rt, b, L, maxM);
    case EditKind::Phase: return launch_phase(rt, b, L, maxM, maxE);
    case EditKind::List: break;
    }
    hipLaunchKernelGGL(k_reduce, dim3((maxM + 255) / 256, R), dim3(256), 0, rt->stream, d_sas);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

}  // namespace ps
