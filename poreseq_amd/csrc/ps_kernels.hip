// ps_kernels.hip — gfx950 kernels for the banded event<->sequence DP (the edit scoring that reads its matrices: ps_edit.hip).
//
// Reference behaviour being reproduced (file:line under the reference tree):
//   updaterefs / getrefstate      cpp/EventData.h:110-183
//   fillColumn / fillColumnBack   cpp/Alignment.cpp:111-274 / :280-444
//   backtrace                     cpp/Alignment.cpp:516-624
//
// Everything is FP64 and compiled with -ffp-contract=off: each cell is computed with the
// reference's operation order, so results are bit-identical to the CPU path (logs / pow are
// taken on the host with the same libm the reference uses).
//
// Execution model.  A DP cell (i, j) (level i, state column j) lives on anti-diagonal s = i + j.
// Storage is skewed: REC[s][i mod P].  One workgroup of P lanes owns one alignment and sweeps
// s = 2 .. n0 + C; lane `slot` owns the row i == slot (mod P) that is inside the band on that
// anti-diagonal (the band's footprint on one anti-diagonal is a contiguous run of at most
// 2W + 1 rows, because the band centre is a monotone function of the column; P is sized from the
// measured footprint, typically ~half the band).  Pipeline per batch of alignments:
//   k_lb / k_lo   band centres per column; lowest / highest in-band row + footprint per anti-diagonal
//   k_fill        emissions, band flags, recurrence, back-pointer codes and column maxima in one sweep
//                 (one 16-byte record + one 2-byte step word per cell leave the chip; nothing is re-read)
//   k_prefix      running MaxInfo per column, first cell of the global maximum
//   k_backtrace   LDS-tile walker with wave-wide look-ahead and tile prefetch, then k_fill_like, k_updaterefs /
//                 k_lb for the new band centres
#include <algorithm>
#include <atomic>

#include "ps_internal.h"
#include "ps_slowmask.h"
#include "ps_dev.h"

namespace ps {

__device__ __forceinline__ int slot_of(int i, int P) { return i % P; }

// ------------------------------------------------------------------------------------------------
// updaterefs: ref_align -> ref_index, refstart, refend   (cpp/EventData.h:110-169)
// one 256-thread block per job; each thread owns a contiguous chunk of levels
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_updaterefs(BatchD b) {
    const JobD& J = b.jobs[blockIdx.x];
    JobOut* O = J.out;
    const int n = J.n0, tid = threadIdx.x;
    const double* __restrict__ ra = J.ra;
    double* __restrict__ ri = J.ri;
    __shared__ int s_first[256], s_last[256];
    const int chunk = (n + 255) / 256;
    const int t0 = min(n, tid * chunk), t1 = min(n, t0 + chunk);
    int first = 0x7fffffff, last = -1;
    for (int t = t0; t < t1; t++)
        if (ra[t] > 0) { if (first == 0x7fffffff) first = t; last = t; }
    s_first[tid] = first; s_last[tid] = last;
    __syncthreads();
    int a0 = 0x7fffffff, a1 = -1, prev = -1, next = 0x7fffffff;
    for (int k = 0; k < 256; k++) {
        a0 = min(a0, s_first[k]); a1 = max(a1, s_last[k]);
        if (k < tid) prev = max(prev, s_last[k]);
        if (k > tid) next = min(next, s_first[k]);
    }
    if (a1 < 0) {
        if (tid == 0) { O->has_index = 0; O->refstart = -1; O->refend = -1; }
        return;
    }
    if (tid == 0) { O->has_index = 1; O->refstart = (int)ra[a0]; O->refend = (int)ra[a1]; }
    const double slope = (ra[a1] - ra[a0]) / (double)(a1 - a0);
    const double icpt = ra[a0] - slope * (double)a0;
    int lastal = prev;
    for (int t = t0; t < t1; t++) {
        const double v = ra[t];
        if (t < a0 || t > a1) {
            ri[t] = slope * (double)t + icpt;
        } else if (v > 0) {
            ri[t] = v;
            lastal = t;
        } else {
            // inside [a0, a1], not aligned: interpolate between neighbours unless the left anchor is level 0 (sic)
            int nx = t + 1;
            while (nx < t1 && !(ra[nx] > 0)) nx++;
            if (nx >= t1) nx = next;
            if (lastal > 0) {
                const double mm = (ra[nx] - ra[lastal]) / (double)(nx - lastal);
                ri[t] = mm * (double)(t - lastal) + ra[lastal];
            } else {
                ri[t] = v;
            }
        }
    }
}

// lb[j] = getrefstate(j) for j = 0 .. lbn-1 (or -1 when ref_index is empty)
__global__ void k_lb(BatchD b, int which) {
    const JobD& J = b.jobs[blockIdx.y];
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= J.lbn) return;
    int* lb = b.lb + (which ? J.lbn_off : J.lb_off);
    lb[j] = J.out->has_index ? lower_bound_d(J.ri, J.n0, j) : -1;
}

// ------------------------------------------------------------------------------------------------
// lo[s] / hi[s]: lowest and highest in-band row on anti-diagonal s (-1: none).
// The columns present on s are those with i0(j) + j <= s <= i1(j) + j — a contiguous range
// [jlo, jhi] because both bounds are strictly increasing in j; rows are s - j, so lo = s - jhi,
// hi = s - jlo and the footprint hi - lo + 1 <= 2W + 1.  The per-job maximum footprint sizes P.
// Consecutive non-empty anti-diagonals move each end by at most one row (jhi and jlo grow by at most one per
// step), which is what lets k_fill derive every band flag from these two numbers and the lane's own history.
// Entries [S, S + LO_PAD) are -1: the fill pipeline looks a few anti-diagonals past the end.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_lo(BatchD b, int ndir) {
    const int jd = blockIdx.y, job = jd / ndir, dir = jd % ndir;
    const JobD& J = b.jobs[job];
    if (J.out->inert) return;
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int width = 0;
    if (s < J.S + LO_PAD) {
        const int* lb = b.lb + J.lb_off;
        int res = -1, top = -1;
        if (J.C >= 1 && s < J.S) {
            int i0, i1;
            band_of(lb, dir, 1, J.C, J.n0, J.W, i0, i1);
            if (i0 + 1 <= s) {
                int lo = 1, hi = J.C;  // largest j with i0(j) + j <= s
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    band_of(lb, dir, mid, J.C, J.n0, J.W, i0, i1);
                    if ((int64_t)i0 + mid <= s) lo = mid; else hi = mid - 1;
                }
                const int jhi = lo;
                band_of(lb, dir, J.C, J.C, J.n0, J.W, i0, i1);
                if ((int64_t)i1 + J.C >= s) {
                    lo = 1; hi = J.C;  // smallest j with i1(j) + j >= s
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        band_of(lb, dir, mid, J.C, J.n0, J.W, i0, i1);
                        if ((int64_t)i1 + mid >= s) hi = mid; else lo = mid + 1;
                    }
                    if (lo <= jhi) { res = (int)(s - jhi); top = (int)(s - lo); width = jhi - lo + 1; }
                }
            }
        }
        (b.lo + J.lo_off[dir])[s] = res;
        (b.hi + J.lo_off[dir])[s] = top;
    }
    for (int off = 32; off; off >>= 1) width = max(width, __shfl_xor(width, off));
    if ((threadIdx.x & 63) == 0 && width > 0) atomicMax(b.maxw, width);   // one P for the whole batch
}

// ------------------------------------------------------------------------------------------------
// k_fill: the whole of fillColumn / fillColumnBack (cpp/Alignment.cpp:111-274 / 280-444) for one alignment and
// direction in one pass — emission log-densities, band flags, the recurrence, the back-pointer codes (forward) and
// the per-column maxima — so a DP cell costs one 16-byte record (+ a 2-byte step word forward) of HBM traffic and
// nothing is re-read.
//
// One workgroup of P lanes per (job, direction) sweeps the anti-diagonals s = i + j.  Lane `slot` holds the row
// i == slot (mod P) that is inside [lo(s), lo(s) + P); its cell on anti-diagonal s is (i, s - i), so a lane walks
// along one row, one column per step, until lo passes the row, then takes row i + P.  What a cell needs:
//   (i, j-1)    the lane's own previous value (cm);
//   (i-1, j)    what the lane one slot up published on the previous anti-diagonal  -> two LDS exchange buffers,
//               written and read alternately, one LDS-only s_barrier per anti-diagonal;
//   (i-1, j-1)  what that lane published two anti-diagonals ago = what this lane read one step earlier (dm).
// A lane without a cell holds and publishes -infinity: read as the upper neighbour that is the top-row rule (no stay /
// extend / insert into a band's first row), read as the left neighbour max(., 0) turns it into the reference's
// "implicit zero" for neighbours outside the previous band (cpp/Alignment.cpp:201-225; real scores are >= 0).
// Band flags come from lo / hi and the lane's own history instead of per-cell band lookups:
//   in band        lo <= i <= hi
//   top row        i == lo on an anti-diagonal where a new column starts (lo did not move)
//   left valid     the lane's previous cell (same row, previous column) was in band, or this is column 1
//   diag valid     the reference tests ROW i against the previous band (p0 < i <= p1): previous cell in band and
//                  not that band's top row; the value is read as zero when the previous column is an invalid 5-mer
// Values are computed with v_max chains (the maximum does not depend on the reference's tie order); the forward
// step codes then follow from equality tests against the final value, which reproduce the ordered strict-'>'
// selection of cpp/Alignment.cpp:240-267 (the first candidate, in the reference's order, that equals the maximum).
//
// Divisions.  The three divisors of an emission (cpp/AlignUtil.h:34-53) are table values: the 5-mer's level stdv and sd
// mean, and the level's own stdv.  Their correctly rounded reciprocals y = RN(1/b) are tabulated (host IEEE division) and
// a/b is formed as  q0 = a*y; r = fma(-b,q0,a); q1 = fma(r,y,q0); r = fma(-b,q1,a); q = fma(r,y,q1)  — Markstein's
// sequence, whose last step is provably the correctly rounded quotient given y = RN(1/b) and a faithful q1 (Markstein 1990;
// Muller et al., Handbook of Floating-Point Arithmetic, section 4.7): bit-identical to the reference's IEEE division at 5
// instructions instead of ~13 (no v_rcp_f64 / v_div_*).  The host enables it per AlignData only when every table value lies in
// the range of ps_sane.h, which bounds the numerators as well (an infinite or subnormal numerator breaks the sequence); otherwise
// the kernel divides.  tests/test_fastdiv.py checks the sequence against IEEE division on 10^8 operand pairs, including all-ones
// and power-of-two significands; tests/native/emission_check.cpp the whole emission over the corners of the accepted range.
//
// Software pipeline (everything that does not depend on a neighbour runs ahead of the recurrence):
//   windows, 4-step groups  5-mer states of the lane's next four columns (one 16-byte load) and the level record of its
//                           row, fetched at least three steps before first use.  A lane keeps its row for the whole window
//                           or idles: P exceeds the widest footprint by 9, so between two rows a lane idles 9 steps;
//   model row, 3 ahead      64-byte row {mean, 1/stdv, stdv, log stdv, sd mean, 1/sd mean, lambda, log lambda} of the
//                           column's 5-mer from LDS (64 KB per event);
//   emission, 2 ahead       ~30 FP64 instructions;
//   recurrence              exchange read, ~10 additions, max chain, codes, coalesced stores, exchange write.
// Bodies of 8 anti-diagonals near one on which the band resumes after an empty stretch (in practice: the start of the
// sweep) — rows may then jump by any amount and take a cell at once — run a SLOW variant that recomputes rows exactly
// and loads states / levels directly; every value is the same in both variants.
// Column maxima (MaxInfo per column) go through an LDS ring of ds_max and are flushed to memory as columns complete.
// ------------------------------------------------------------------------------------------------
// one bit per anti-diagonal of a 64-step chunk (lane k holds lo of step k, `before` = lo of the step before the chunk): the
// band resumes there after an empty stretch (lo(t-1) < 0 <= lo(t))
__device__ __forceinline__ unsigned long long resume_bits(int lov, int before) {
    const int prev = __builtin_amdgcn_update_dpp(before, lov, 0x138 /*wave_shr:1*/, 0xf, 0xf, false);
    return __ballot(lov >= 0 && prev < 0);
}
// resume_spread(): which 8-step bodies the resumes of one chunk make SLOW (ps_slowmask.h, host-tested)

constexpr int FB = 8;            // anti-diagonals per loop body
constexpr int FCH = 64;          // anti-diagonals per chunk: lo / hi prefetch unit, flush interval of the column maxima

template <int DIR>
struct FillState {
    double cm, cs;         // this lane's latest main / stay; -infinity while it has no cell
    double dm, de;         // upper neighbour's main (and, backward, main + emission) as read one step earlier
    double o1, o2;         // emission (+ lik_offset) of this lane's cell one / two anti-diagonals ahead
    bool pin, ptop, pdead; // the lane's previous anti-diagonal: had a cell position in band / was the band's top row / invalid 5-mer
    int row;               // the lane's row
    int stq[4];            // states of the lane's column on anti-diagonals s .. s + 3
    int stw[2][4];         // state windows (two groups in flight)
    double lv[2][4];       // level windows {level mean, level stdv, 3 log stdv, 1 / level stdv}
    double mr[8];          // model row of the lane's column on anti-diagonal s + 2 (read from LDS one step earlier)
};

struct FillCtx {
    PS_GLOBAL const v4d* lev;     // level records of this direction: [row - 1] = {mean, stdv, 3 log stdv, 1 / stdv}
    gcip st;
    gcip LO; gcip HI;
    PS_GLOBAL char* rec; PS_GLOBAL char* flg;   // anti-diagonal 0 of the job's matrix (uniform); lanes add their slot offset
    unsigned rec_off, flg_off;    // this lane's byte offset inside an anti-diagonal
    const char* mdl;              // LDS: model rows [NS][8]
    char* xch;                    // LDS: two exchange buffers of P records
    char* ring;                   // LDS: column maxima, ringmask + 1 bytes
    unsigned ringmask;
    int P, n0, C, slot, S;
    int wa[2], ra[2];             // byte offsets of this lane's / its upper neighbour's record in the two buffers
    double lsk, lst, lex, lin, off, log2pi;
};

template <bool FASTDIV>
__device__ __forceinline__ double fill_emission(const FillCtx& c, const double (&m)[8], const double (&lev)[4]) {
    return emission8<FASTDIV>(m, lev, c.log2pi, c.off);
}

// Model rows in LDS, two layouts:
//  * 80 bytes apart (the host's layout, copied as is).  With 64 the k-th quarter of every row falls on 4 of the 16 four-bank
//    groups (ds_read_b128 of 64 random rows: 71 % conflict cycles measured), with 80 on all 16.
//  * CMP (compact): 64 bytes apart, quarter k of row r stored in quarter k ^ ((r >> 2) & 3) — the same 16 groups in 64 KB
//    instead of 80, at 5 more VALU instructions per step.  With it a lone sweep of up to 384 lanes (256 backward) takes
//    at most half of a CU's 160 KB of LDS, so two workgroups share a CU.
template <bool CMP>
__device__ __forceinline__ void fill_model_row(const FillCtx& c, int state, double (&m)[8]) {
    const int st0 = state < 0 ? 0 : state;
    double2 a, bq, cq, dq;
    if (CMP) {
        const unsigned q0 = ((unsigned)st0 << 6) | (((unsigned)st0 << 2) & 0x30u);
        a = *(const double2*)(c.mdl + q0); bq = *(const double2*)(c.mdl + (q0 ^ 16u));
        cq = *(const double2*)(c.mdl + (q0 ^ 32u)); dq = *(const double2*)(c.mdl + (q0 ^ 48u));
    } else {
        const char* row = c.mdl + __umul24((unsigned)st0, (unsigned)MODEL_ROW_BYTES);   // v_mul_u32_u24: full rate (the compiler's v_mul_lo_u32 for (s << 6) + (s << 4) is not)
        a = *(const double2*)row; bq = *(const double2*)(row + 16); cq = *(const double2*)(row + 32); dq = *(const double2*)(row + 48);
    }
    m[0] = a.x; m[1] = a.y; m[2] = bq.x; m[3] = bq.y; m[4] = cq.x; m[5] = cq.y; m[6] = dq.x; m[7] = dq.y;
}

__device__ __forceinline__ void fill_levels(const FillCtx& c, int i, double (&lev)[4]) {
    const v4d v = c.lev[clampi(i, 1, c.n0) - 1];
    lev[0] = v.x; lev[1] = v.y; lev[2] = v.z; lev[3] = v.w;
}
// index of the state of the lane's column on anti-diagonal t, row i (out-of-range columns read the -1 padding;
// windows read [idx, idx + 3])
template <int DIR>
__device__ __forceinline__ int fill_state_index(const FillCtx& c, int t, int i) {
    const int j = t - i;
    const int idx = DIR == 0 ? j - 1 : c.C - j;
    return clampi(idx, -3, c.C - 1);
}
// row of residue class `slot` inside [lo, lo + P)
__device__ __forceinline__ int fill_row_of(const FillCtx& c, int lo) {
    int d = (c.slot - lo) % c.P;
    if (d < 0) d += c.P;
    return lo + d;
}

// One anti-diagonal.  PH = position in the loop body (compile time): exchange buffer, window set, state queue slot.
template <int DIR, int PH, bool SLOW, bool FASTDIV, bool CMP>
__device__ __forceinline__ void fill_step(FillState<DIR>& r, const FillCtx& c, const int s, const int lo_s, const int hi_s,
                                          const bool newcol /* uniform: a column starts on this anti-diagonal */) {
    const double NINF = -__builtin_inf();
    constexpr int G = PH >> 2, K = PH & 3;
    // ---- exchange read: what the lane one slot up published on the previous anti-diagonal
    double um, us, ue = 0.0;
    {
        const char* p = c.xch + c.ra[(PH & 1) ^ 1];
        if (DIR == 0) { const double2 u = *(const double2*)p; um = u.x; us = u.y; }
        else { um = *(const double*)p; us = *(const double*)(p + 8); ue = *(const double*)(p + 16); }
    }
    // ---- the lane's row and band flags on this anti-diagonal
    int i = r.row;
    {
        const bool behind = lo_s >= 0 && i < lo_s;
        if (!SLOW) i = behind ? i + c.P : i;     // lo moves one row per step at most: one slot's row falls out of [lo, lo + P)
        else if (behind) i = fill_row_of(c, lo_s);
        r.row = i;
    }
    const bool inb = lo_s >= 0 && i <= hi_s;
    const bool top = inb && newcol && i == lo_s;
    const bool first = s - i == 1;
    const bool dead = r.stq[K] < 0;
    // ---- windows: at a group start fetch the states / levels of anti-diagonals s + 6 .. s + 9 (a window = 4w .. 4w+3; s0 == 2 mod 8)
    if (K == 0) {
        const int t0 = s + 6;
        if (DIR == 0) {
            const int a = fill_state_index<0>(c, t0, i);           // ascending with the anti-diagonal
            const v4i v = *(const PS_GLOBAL v4i_a4*)(c.st + a);    // 4-byte aligned 16-byte load
            r.stw[G][0] = v.x; r.stw[G][1] = v.y; r.stw[G][2] = v.z; r.stw[G][3] = v.w;
        } else {
            const int a = fill_state_index<1>(c, t0 + 3, i);       // descending: element 3 - k belongs to step t0 + k
            const v4i v = *(const PS_GLOBAL v4i_a4*)(c.st + a);
            r.stw[G][0] = v.w; r.stw[G][1] = v.z; r.stw[G][2] = v.y; r.stw[G][3] = v.x;
        }
        fill_levels(c, i, r.lv[G]);
    }
    // ---- emission of anti-diagonal s + 2: its model row arrived during the previous step; levels from the window the
    //      previous group start fetched (set G ^ 1)
    double o_new;
    {
        if (!SLOW) o_new = fill_emission<FASTDIV>(c, r.mr, r.lv[G ^ 1]);
        else {
            const int lo2 = (s + 2 >= 0 && s + 2 < c.S) ? c.LO[s + 2] : -1;
            double lev[4];
            fill_levels(c, lo2 >= 0 ? fill_row_of(c, lo2) : i, lev);
            o_new = fill_emission<FASTDIV>(c, r.mr, lev);
        }
    }
    __builtin_amdgcn_sched_barrier(0);   // stage fence: with three waves per SIMD the other waves hide latency; keeping the
                                         // stages apart keeps their temporaries from piling up (168 VGPRs for 12 waves per CU)
    // ---- model row of anti-diagonal s + 3: its state is element (PH + 1) & 3 of the window [4w, 4w+3] holding s + 3,
    //      fetched at body offset 4w - 6: the previous body's second group (set 1), this body's first (0) or second (1).
    //      (Handing the rows down the lanes with DPP instead of gathering them — lane L+1 needs on step s+1 the row lane L
    //      used on step s — removes the LDS bank conflicts of the gather, 71 % of the LDS cycles, but costs 16 more VALU
    //      instructions per step and the kernel is VALU-issue bound: measured 13.3 ms against 12.2 ms per 10 kb fill.)
    {
        constexpr int SET = (PH <= 2 || PH == 7) ? 1 : 0;
        int state = r.stw[SET][(PH + 1) & 3];
        if (SLOW) {
            const int lo3 = (s + 3 >= 0 && s + 3 < c.S) ? c.LO[s + 3] : -1;
            state = c.st[fill_state_index<DIR>(c, s + 3, lo3 >= 0 ? fill_row_of(c, lo3) : i)];
        }
        r.stq[(PH + 3) & 3] = state;
        fill_model_row<CMP>(c, state, r.mr);
    }
    __builtin_amdgcn_sched_barrier(0);
    // ---- recurrence on anti-diagonal s
    {
        const bool vd = first || (r.pin && !r.ptop);
        const bool rd = !first && r.pin && !r.ptop && !r.pdead;
        const double o = r.o1;
        double L;   // max(cm, 0) in one instruction (fmax() would first canonicalise its operand)
        asm("v_max_f64 %0, %1, 0" : "=v"(L) : "v"(r.cm));
        const double D = rd ? r.dm : 0.0;
        const double cSTAY = DIR == 0 ? um + o + c.lst : ue + c.lst;       // backward: (main + emission) of the cell above
        const double cEXT = DIR == 0 ? us + o + c.lex : us + c.lex;         // backward: `us` carries stay + emission
        const double cINS = um + c.lin;
        const double cSKIP = L + c.lsk;
        const double cMATCH = DIR == 0 ? D + o : (rd ? r.de : 0.0);
        const double cIGN = D + c.lin;
        const double floor_s = top ? -BIG : 0.0;
        double ns = fmax(floor_s, cSTAY);
        ns = fmax(ns, cEXT);
        double nm = fmax(0.0, cSKIP);
        nm = fmax(nm, cMATCH);
        nm = fmax(nm, cINS);
        nm = fmax(nm, cIGN);
        nm = fmax(nm, ns);
        const bool act = inb && !dead;
        r.cm = act ? nm : NINF;
        r.cs = act ? ns : NINF;
        // stored record: the cell; zeros for a cell of an invalid-5-mer column (cpp/Alignment.cpp:162-163) and, harmlessly,
        // for slots outside the band (nm >= 0, and the stay value of a top row is -1e300 and must stay so)
        double rx;
        asm("v_max_f64 %0, %1, 0" : "=v"(rx) : "v"(r.cm));
        // (a half whose sweep is shorter than its partner's keeps stepping: its idle records go to the last padding row)
        const uint64_t sP = (uint64_t)(unsigned)(min(s, c.S + MAT_BACK - 1) + MAT_FRONT) * (unsigned)c.P;   // uniform
        *(PS_GLOBAL v2d*)(c.rec + sP * 16 + c.rec_off) = (v2d){rx, act ? ns : 0.0};
        if (DIR == 0) {
            // back-pointer codes: stay matrix STAY then EXTEND with strict '>', main matrix in the reference's order
            unsigned ss = cSTAY > floor_s ? M_STAY : 0u;
            ss = cEXT > fmax(floor_s, cSTAY) ? M_EXTEND : ss;
            unsigned sm = M_STAY;
            sm = cIGN == nm ? M_IGNORE : sm;
            sm = cINS == nm ? M_INSERT : sm;
            sm = cMATCH == nm ? (vd ? M_MATCH : M_IMPL) : sm;
            sm = cSKIP == nm ? M_SKIP : sm;
            sm = nm > 0.0 ? sm : 0u;
            // bits 14 / 15: main / stay score <= 0 (the backtrace stops there, cpp/Alignment.cpp:542)
            const unsigned w = sm | (ss << 8) | (nm > 0.0 ? 0u : 0x4000u) | (ns > 0.0 ? 0u : 0x8000u);
            *(PS_GLOBAL unsigned short*)(c.flg + sP * 2 + c.flg_off) = (unsigned short)(act ? w : FLG_DEAD);
        }
        // publish for the lane one slot down
        char* q = c.xch + c.wa[PH & 1];
        if (DIR == 0) {
            *(double2*)q = make_double2(r.cm, r.cs);
        } else {
            *(double*)q = r.cm; *(double*)(q + 8) = r.cs + o; *(double*)(q + 16) = r.cm + o;
        }
        // column maximum (scores are >= 0: their bit patterns order like unsigned integers; 0 is a no-op)
        atomicMax((unsigned long long*)(c.ring + (((unsigned)(s - i) << 3) & c.ringmask)), (unsigned long long)__double_as_longlong(rx));
        r.dm = um; r.de = ue;
        r.pin = inb; r.ptop = top; r.pdead = dead;
    }
    r.o1 = r.o2; r.o2 = o_new;
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

template <int DIR, bool SLOW, bool FASTDIV, bool CMP>
__device__ __forceinline__ void fill_group8(FillState<DIR>& r, const FillCtx& c, const int s0, const int (&lov)[FB], const int (&hiv)[FB], const int lo_p) {
#define PS_NEWCOL(k, prev) ((prev) < 0 || lov[k] == (prev))
    fill_step<DIR, 0, SLOW, FASTDIV, CMP>(r, c, s0 + 0, lov[0], hiv[0], PS_NEWCOL(0, lo_p));
    fill_step<DIR, 1, SLOW, FASTDIV, CMP>(r, c, s0 + 1, lov[1], hiv[1], PS_NEWCOL(1, lov[0]));
    fill_step<DIR, 2, SLOW, FASTDIV, CMP>(r, c, s0 + 2, lov[2], hiv[2], PS_NEWCOL(2, lov[1]));
    fill_step<DIR, 3, SLOW, FASTDIV, CMP>(r, c, s0 + 3, lov[3], hiv[3], PS_NEWCOL(3, lov[2]));
    fill_step<DIR, 4, SLOW, FASTDIV, CMP>(r, c, s0 + 4, lov[4], hiv[4], PS_NEWCOL(4, lov[3]));
    fill_step<DIR, 5, SLOW, FASTDIV, CMP>(r, c, s0 + 5, lov[5], hiv[5], PS_NEWCOL(5, lov[4]));
    fill_step<DIR, 6, SLOW, FASTDIV, CMP>(r, c, s0 + 6, lov[6], hiv[6], PS_NEWCOL(6, lov[5]));
    fill_step<DIR, 7, SLOW, FASTDIV, CMP>(r, c, s0 + 7, lov[7], hiv[7], PS_NEWCOL(7, lov[6]));
#undef PS_NEWCOL
}

constexpr int FILL_MODEL_BYTES = MODEL_ROW_BYTES * NS;

// One half of a k_fill workgroup: the sweep of one (job, direction).  `slot` is the thread's lane inside the half, `hsm` the
// half's private LDS (exchange buffers, ring, bitmap), `model` the workgroup's shared model rows, Smax the longer of the two
// sweeps of the workgroup (both halves execute the same number of barriers).
template <int DIR, bool FASTDIV, bool CMP>
__device__ __forceinline__ void fill_body(const BatchD& b, const JobD& J, const char* model, char* hsm, const int slot, const int Smax,
                                          const int rcols, const int slowwords) {
    const int P = uni(J.P);
    FillCtx c;
    c.lev = (PS_GLOBAL const v4d*)uni_ptr(J.lev[DIR]); c.st = (gcip)uni_ptr(J.st);
    c.LO = (gcip)uni_ptr(b.lo + J.lo_off[DIR]); c.HI = (gcip)uni_ptr(b.hi + J.lo_off[DIR]);
    c.rec = (PS_GLOBAL char*)uni_ptr(b.rec + J.mat_off[DIR] - (int64_t)MAT_FRONT * P); c.flg = (PS_GLOBAL char*)uni_ptr(b.flg + J.mat_off[DIR] - (int64_t)MAT_FRONT * P);
    c.rec_off = (unsigned)slot * 16u; c.flg_off = (unsigned)slot * 2u;
    c.P = P; c.n0 = uni(J.n0); c.C = uni(J.C); c.slot = slot;
    c.lsk = J.lsk; c.lst = J.lst; c.lex = J.lex; c.lin = J.lin; c.off = J.lik_offset; c.log2pi = b.log2pi;
    constexpr int RB = DIR ? 24 : 16;   // bytes per exchanged record: {main, stay} / {main, stay + em, main + em}
    c.mdl = model;
    c.xch = hsm;
    c.ring = c.xch + 2 * P * (CMP ? RB : 24);   // (a half of a pair may run either direction: sized for the larger record)
    c.ringmask = (unsigned)rcols * 8u - 1u;
    unsigned* slowmap = (unsigned*)(c.ring + rcols * 8);   // (!CMP) one bit per 8-step body: it runs the SLOW variant
    for (int k = slot; k < rcols; k += P) ((unsigned long long*)c.ring)[k] = 0ull;
    if (!CMP) for (int k = slot; k < slowwords; k += P) slowmap[k] = 0u;
    const int up_slot = slot == 0 ? P - 1 : slot - 1;
    const double NINF = -__builtin_inf();
#pragma unroll
    for (int k = 0; k < 2; k++) {
        c.wa[k] = (k * P + slot) * RB;
        c.ra[k] = (k * P + up_slot) * RB;
        *(double*)(c.xch + c.wa[k]) = NINF; *(double*)(c.xch + c.wa[k] + 8) = NINF;
        if (DIR) *(double*)(c.xch + c.wa[k] + 16) = NINF;
    }
    const int S = uni((int)J.S);                         // this half's sweep; the loops below run to Smax >= S (idle steps past S)
    const int s_first = 2 - FB;                          // the pipeline needs a few steps to fill; they fall into the front padding
    c.S = S;
    __syncthreads();
    // Bodies that must run the SLOW variant: the band resumes on anti-diagonal t (lo(t-1) < 0 <= lo(t)).  Windows fetched on
    // t - 9 .. t - 1 hold the states / levels of rows that may no longer be the lane's; they are consumed on t - 6 .. t + 6:
    // every body holding a step of [t - 6, t + 6] is slow.  The plain layout marks them in an LDS bitmap up front; the compact
    // one has no LDS to spare and derives them from the lo chunks as they stream by (resume_spread).  (One mechanism would do,
    // but the second costs the 168-VGPR pair build 70 spilled registers and 4 % — register allocation, not logic.)
    if (!CMP)
        for (int t = 2 + slot; t < S; t += P) {
            if (c.LO[t] >= 0 && c.LO[t - 1] < 0) {
                const int b0 = max(0, (t - 6 - s_first) >> 3), b1 = (t + 6 - s_first) >> 3;
                for (int bb = b0; bb <= b1; bb++) atomicOr(&slowmap[bb >> 5], 1u << (bb & 31));
            }
        }
    FillState<DIR> r;
    r.cm = NINF; r.cs = NINF; r.dm = NINF; r.de = NINF; r.o1 = 0.0; r.o2 = 0.0;
    r.pin = false; r.ptop = false; r.pdead = false;
    r.row = slot == 0 ? P : slot;   // rows start at 1: the smallest row of this slot's residue class
#pragma unroll
    for (int k = 0; k < 4; k++) r.stq[k] = 0;
#pragma unroll
    for (int g = 0; g < 2; g++) {
#pragma unroll
        for (int k = 0; k < 4; k++) r.stw[g][k] = 0;
        r.lv[g][0] = 0.0; r.lv[g][1] = 1.0; r.lv[g][2] = 0.0; r.lv[g][3] = 1.0;
    }
    r.mr[0] = 0.0; r.mr[1] = 1.0; r.mr[2] = 1.0; r.mr[3] = 0.0; r.mr[4] = 1.0; r.mr[5] = 1.0; r.mr[6] = 0.0; r.mr[7] = 0.0;
    __syncthreads();

    int flushed = 1;                                     // columns below this have their maximum in memory
    double* gcmax = b.cmax + J.col_off[DIR];
    int lo_p = -1;                                       // lo of the previous anti-diagonal
    const int lane = slot & 63;
    // lo / hi of 64 anti-diagonals per VGPR (lane k holds entry k), fetched one chunk ahead
    int loc = c.LO[max(s_first + lane, 0)], hic = c.HI[max(s_first + lane, 0)];
    if (s_first + lane < 0) { loc = -1; hic = -1; }
    // `slow` (CMP): bits 0-7 the bodies of the current chunk, above them what is known of the chunks after (one scalar register)
    unsigned slow = CMP ? __builtin_amdgcn_readfirstlane(resume_spread(resume_bits(loc, -1)) >> 8) : 0u;
    int nbody = 0;
    for (int cb = s_first; cb < Smax; cb += FCH) {
        const int lon = c.LO[min(cb + FCH + lane, S + LO_PAD - 1)], hin = c.HI[min(cb + FCH + lane, S + LO_PAD - 1)];
        if (CMP) slow |= __builtin_amdgcn_readfirstlane(resume_spread(resume_bits(lon, __builtin_amdgcn_readlane(loc, 63))));
#pragma unroll 1
        for (int o = 0; o < FCH && cb + o < Smax; o += FB, nbody++) {
            const int s0 = cb + o;
            int lov[FB], hiv[FB];
#pragma unroll
            for (int k = 0; k < FB; k++) { lov[k] = __builtin_amdgcn_readlane(loc, o + k); hiv[k] = __builtin_amdgcn_readlane(hic, o + k); }
            const unsigned sw = CMP ? slow >> (o >> 3) : __builtin_amdgcn_readfirstlane(slowmap[nbody >> 5]) >> (nbody & 31);
            if (sw & 1u) fill_group8<DIR, true, FASTDIV, CMP>(r, c, s0, lov, hiv, lo_p);
            else fill_group8<DIR, false, FASTDIV, CMP>(r, c, s0, lov, hiv, lo_p);
            lo_p = lov[FB - 1];
        }
        loc = lon; hic = hin;
        slow >>= 8;
        // flush the maxima of completed columns: every column left of the oldest one still present on the next anti-diagonal
        {
            const int sn = cb + FCH;
            const int lo_n = __builtin_amdgcn_readlane(loc, 0), hi_n = __builtin_amdgcn_readlane(hic, 0);
            if (sn < S && lo_n >= 0) {
                const int jdone = sn - hi_n;             // oldest column still present
                for (int col = flushed + slot; col < jdone; col += P) {
                    unsigned long long* e = (unsigned long long*)(c.ring + (((unsigned)col * 8u) & c.ringmask));
                    const unsigned long long v = *e;
                    *e = 0ull;
                    gcmax[col] = __longlong_as_double((long long)v);
                }
                flushed = max(flushed, jdone);
            }
        }
    }
    __syncthreads();
    for (int col = flushed + slot; col <= J.C; col += P)
        gcmax[col] = __longlong_as_double((long long)*(unsigned long long*)(c.ring + (((unsigned)col * 8u) & c.ringmask)));
}

// ------------------------------------------------------------------------------------------------
// k_fill_wide: the same sweep for bands whose footprint does not fit one lane per row (more than 1015 rows on an anti-diagonal:
// realign_width beyond ~500 in the worst case, ~980 for events with one level per base).  Every thread holds TWO slots (t and
// t + blockDim), so a workgroup of up to 1024 threads carries up to 2048 slots (realign_width <= 1022 for any input).  This is the
// plain form of k_fill — no prefetch windows, no software pipeline, model rows read from global memory (two 98 KB exchange buffers
// leave no room for the table in LDS), one sweep per workgroup — i.e. the width is supported, not tuned: ~4x the time per cell.
// Cell arithmetic, flags, codes and column maxima are the same expressions as in fill_step.
// ------------------------------------------------------------------------------------------------
template <int DIR, bool FD>
__device__ __forceinline__ void fill_wide_body(const BatchD& b, const JobD& J, char* smem, const int rcols) {
    constexpr int R = 2;
    const int T = blockDim.x, P = J.P, tid = threadIdx.x, C = J.C, S = (int)J.S;
    const int* __restrict__ LO = b.lo + J.lo_off[DIR];
    const int* __restrict__ HI = b.hi + J.lo_off[DIR];
    double2* __restrict__ rec = b.rec + J.mat_off[DIR];
    unsigned short* __restrict__ flg = b.flg + J.mat_off[DIR];
    const double4* __restrict__ levs = (const double4*)J.lev[DIR];
    const int* __restrict__ st = J.st;
    const char* __restrict__ model = (const char*)J.model8;
    const double lsk = J.lsk, lst = J.lst, lex = J.lex, lin = J.lin, off = J.lik_offset, log2pi = b.log2pi;
    const double NINF = -__builtin_inf();
    double* xch = (double*)smem;                                  // [2][P][3]
    unsigned long long* ring = (unsigned long long*)(smem + (size_t)2 * P * 24);
    const unsigned ringmask = (unsigned)rcols - 1u;
    for (int k = tid; k < 2 * P * 3; k += T) xch[k] = NINF;
    for (int k = tid; k < rcols; k += T) ring[k] = 0ull;
    double cm[R], cs[R], dm[R], de[R];
    int row[R];
    bool pin[R], ptop[R], pdead[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int slot = tid + r * T;
        cm[r] = NINF; cs[r] = NINF; dm[r] = NINF; de[r] = NINF;
        row[r] = slot == 0 ? P : slot;
        pin[r] = false; ptop[r] = false; pdead[r] = false;
    }
    __syncthreads();
    double* gcmax = b.cmax + J.col_off[DIR];
    int lo_p = -1, flushed = 1;
    for (int s = 2; s < S; s++) {
        const int lo = LO[s], hi = HI[s];
        const bool newcol = lo_p < 0 || lo == lo_p;
        const int par = s & 1;
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int slot = tid + r * T;
            int i = row[r];
            if (lo >= 0 && i < lo) {
                i += P;
                if (i < lo) { int d = (slot - lo) % P; if (d < 0) d += P; i = lo + d; }
            }
            row[r] = i;
            const bool inb = lo >= 0 && i <= hi;
            const bool top = inb && newcol && i == lo;
            const int j = s - i;
            const bool first = j == 1;
            const double* up = xch + ((size_t)(par ^ 1) * P + (slot == 0 ? P - 1 : slot - 1)) * 3;
            const double um = up[0], us = up[1], ue = up[2];
            double o = 0.0;
            bool dead = false;
            if (inb) {
                const int state = st[DIR == 0 ? j - 1 : C - j];
                dead = state < 0;
                if (!dead) {
                    const double2* q = (const double2*)(model + (size_t)state * MODEL_ROW_BYTES);
                    const double2 q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
                    const double m[8] = {q0.x, q0.y, q1.x, q1.y, q2.x, q2.y, q3.x, q3.y};
                    const double4 l4 = levs[i - 1];
                    const double lev[4] = {l4.x, l4.y, l4.z, l4.w};
                    o = emission8<FD>(m, lev, log2pi, off);
                }
            }
            const bool vd = first || (pin[r] && !ptop[r]);
            const bool rd = !first && pin[r] && !ptop[r] && !pdead[r];
            double L;
            asm("v_max_f64 %0, %1, 0" : "=v"(L) : "v"(cm[r]));
            const double D = rd ? dm[r] : 0.0;
            const double cSTAY = DIR == 0 ? um + o + lst : ue + lst;
            const double cEXT = DIR == 0 ? us + o + lex : us + lex;
            const double cINS = um + lin;
            const double cSKIP = L + lsk;
            const double cMATCH = DIR == 0 ? D + o : (rd ? de[r] : 0.0);
            const double cIGN = D + lin;
            const double floor_s = top ? -BIG : 0.0;
            double ns = fmax(floor_s, cSTAY);
            ns = fmax(ns, cEXT);
            double nm = fmax(0.0, cSKIP);
            nm = fmax(nm, cMATCH);
            nm = fmax(nm, cINS);
            nm = fmax(nm, cIGN);
            nm = fmax(nm, ns);
            const bool act = inb && !dead;
            cm[r] = act ? nm : NINF;
            cs[r] = act ? ns : NINF;
            double rx;
            asm("v_max_f64 %0, %1, 0" : "=v"(rx) : "v"(cm[r]));
            const int64_t cell = (int64_t)s * P + slot;
            rec[cell] = make_double2(rx, act ? ns : 0.0);
            if (DIR == 0) {
                unsigned ss = cSTAY > floor_s ? M_STAY : 0u;
                ss = cEXT > fmax(floor_s, cSTAY) ? M_EXTEND : ss;
                unsigned sm = M_STAY;
                sm = cIGN == nm ? M_IGNORE : sm;
                sm = cINS == nm ? M_INSERT : sm;
                sm = cMATCH == nm ? (vd ? M_MATCH : M_IMPL) : sm;
                sm = cSKIP == nm ? M_SKIP : sm;
                sm = nm > 0.0 ? sm : 0u;
                const unsigned w = sm | (ss << 8) | (nm > 0.0 ? 0u : 0x4000u) | (ns > 0.0 ? 0u : 0x8000u);
                flg[cell] = (unsigned short)(act ? w : FLG_DEAD);
            }
            double* mine = xch + ((size_t)par * P + slot) * 3;
            if (DIR == 0) { mine[0] = cm[r]; mine[1] = cs[r]; }
            else { mine[0] = cm[r]; mine[1] = cs[r] + o; mine[2] = cm[r] + o; }
            if (act && rx > 0.0) atomicMax(&ring[(unsigned)j & ringmask], (unsigned long long)__double_as_longlong(rx));
            dm[r] = um; de[r] = ue;
            pin[r] = inb; ptop[r] = top; pdead[r] = dead;
        }
        lo_p = lo;
        __syncthreads();
        if ((s & 63) == 63 && s + 1 < S) {   // flush the maxima of completed columns (left of the oldest column still present)
            const int lo_n = LO[s + 1];
            if (lo_n >= 0) {
                const int jdone = s + 1 - HI[s + 1];
                for (int col = flushed + tid; col < jdone; col += T) {
                    const unsigned long long v = ring[(unsigned)col & ringmask];
                    ring[(unsigned)col & ringmask] = 0ull;
                    gcmax[col] = __longlong_as_double((long long)v);
                }
                flushed = max(flushed, jdone);
            }
            __syncthreads();
        }
    }
    __syncthreads();
    for (int col = flushed + tid; col <= C; col += T) gcmax[col] = __longlong_as_double((long long)ring[(unsigned)col & ringmask]);
}

template <bool FD>
__global__ __launch_bounds__(1024) void k_fill_wide(BatchD b, int ndir, int rcols) {
    extern __shared__ double2 fill_smem[];
    const int jd = blockIdx.x, job = jd / ndir, dir = jd % ndir;
    const JobD& J = b.jobs[job];
    if (J.out->inert) return;
    if (dir == 0) fill_wide_body<0, FD>(b, J, (char*)fill_smem, rcols); else fill_wide_body<1, FD>(b, J, (char*)fill_smem, rcols);
}

// the barrier sequence of fill_body for a half without a sweep (no partner, or an inert job)
__device__ __forceinline__ void fill_idle(const int Smax) {
    __syncthreads();
    __syncthreads();
    const int s_first = 2 - FB;
    for (int cb = s_first; cb < Smax; cb += FCH)
        for (int o = 0; o < FCH && cb + o < Smax; o += FB)
#pragma unroll
            for (int k = 0; k < FB; k++) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    __syncthreads();
}

// One workgroup = up to two sweeps (halves of P lanes each) over the SAME event, so that one model table in LDS (80 KB) serves
// both: the forward and backward fill of an alignment, or two candidate sequences against one event.  With P = 320 / 384 that is
// 10 / 12 waves = 3 per SIMD: the four SIMDs carry equal instruction streams and one wave's exchange / barrier latency is covered
// by the other two (a lone sweep's 5-6 waves leave one SIMD with two waves and the others waiting for it).
// pairs[2 * blockIdx.x + h] = job * ndir + dir of half h, or -1.  PAIR = false: one sweep per workgroup (P > 384, launches of at
// most PAIR_MIN_SWEEPS sweeps, forward sweeps whose events all differ).  CMP: the compact LDS layout of fill_model_row, lone sweeps
// of up to 256 lanes (two workgroups per CU).
// FASTDIV: tabulated reciprocals (the normal case) or IEEE divisions (some divisor of the AlignData is not a sane number)
template <int MAXT, bool PAIR, bool FASTDIV, bool CMP>
__global__ __launch_bounds__(MAXT) void k_fill(BatchD b, const int* __restrict__ pairs, int ndir, int P, int rcols, int slowwords, int halfbytes) {
    static_assert(!(PAIR && CMP), "the compact layout is for lone sweeps");
    extern __shared__ double2 fill_smem[];
    char* smem = (char*)fill_smem;
    constexpr int MODEL_LDS = CMP ? 64 * NS : FILL_MODEL_BYTES;
    const int hw = PAIR ? (int)threadIdx.x / P : 0;
    const int slot = (int)threadIdx.x - hw * P;
    const int jdA = pairs[2 * blockIdx.x], jdB = PAIR ? pairs[2 * blockIdx.x + 1] : -1;
    const bool okA = jdA >= 0 && !b.jobs[jdA / ndir].out->inert, okB = jdB >= 0 && !b.jobs[jdB / ndir].out->inert;
    if (!okA && !okB) return;
    const int Smax = max(okA ? (int)b.jobs[jdA / ndir].S : 0, okB ? (int)b.jobs[jdB / ndir].S : 0);
    {   // the event's model rows (laid out by the host, 80 bytes apart): one copy for the workgroup
        const double2* src = (const double2*)b.jobs[(okA ? jdA : jdB) / ndir].model8;
        double2* dst = (double2*)smem;
        if (CMP) {
            for (int k = threadIdx.x; k < 4 * NS; k += blockDim.x) {
                const int row = k >> 2, q = k & 3;
                dst[(row << 2) | (q ^ ((row >> 2) & 3))] = src[row * 5 + q];
            }
        } else {
            for (int k = threadIdx.x; k < FILL_MODEL_BYTES / 16; k += blockDim.x) dst[k] = src[k];
        }
    }
    const int jd = hw == 0 ? jdA : jdB;
    if (!(hw == 0 ? okA : okB)) { fill_idle(Smax); return; }
    const JobD& J = b.jobs[jd / ndir];
    char* hsm = smem + MODEL_LDS + hw * halfbytes;
    if (jd % ndir == 0) fill_body<0, FASTDIV, CMP>(b, J, smem, hsm, slot, Smax, rcols, slowwords);
    else fill_body<1, FASTDIV, CMP>(b, J, smem, hsm, slot, Smax, rcols, slowwords);
}

// prefix max over columns + (fwd) the first cell achieving the global max ; grid njobs*ndir, block 64
__global__ __launch_bounds__(64) void k_prefix(BatchD b, int ndir) {
    chain_priority();
    const int jd = blockIdx.x, job = jd / ndir, dir = jd % ndir;
    const JobD& J = b.jobs[job];
    const double* cmax = b.cmax + J.col_off[dir];
    double* pm = b.pm + J.col_off[dir];
    const int lane = threadIdx.x;
    double carry = 0.0;
    if (lane == 0) pm[0] = 0.0;
    for (int c0 = 1; c0 <= J.C; c0 += 64) {
        const int c = c0 + lane;
        double v = c <= J.C ? cmax[c] : 0.0;
        for (int off = 1; off < 64; off <<= 1) {
            const double o = __shfl_up(v, off);
            if (lane >= off && o > v) v = o;
        }
        if (carry > v) v = carry;
        if (c <= J.C) pm[c] = v;
        carry = __shfl(v, 63);
    }
    if (dir == 0 && J.K == 0) {   // (strip sweeps hand in their best cell themselves: k_best)
        const double best = carry;
        int bj = 0x7fffffff;
        if (best > 0.0)
            for (int c = 1 + lane; c <= J.C; c += 64)
                if (cmax[c] == best) { bj = c; break; }
        for (int off = 32; off; off >>= 1) bj = min(bj, __shfl_xor(bj, off));
        int bi = 0x7fffffff;
        if (best > 0.0) {  // first row of that column holding the maximum (row-ascending visit order)
            const int* lb = b.lb + J.lb_off;
            const double2* __restrict__ rec = b.rec + J.mat_off[0];
            int i0, i1;
            band_of(lb, 0, bj, J.C, J.n0, J.W, i0, i1);
            for (int i = i0 + lane; i <= i1; i += 64)
                if (rec[(int64_t)(i + bj) * J.P + slot_of(i, J.P)].x == best) { bi = i; break; }
            for (int off = 32; off; off >>= 1) bi = min(bi, __shfl_xor(bi, off));
        }
        if (lane == 0) {
            JobOut* O = J.out;
            O->best = best;
            if (best > 0.0) { O->bj = bj; O->bi = bi; }
            else { O->bj = 0; O->bi = 0; }
        }
    }
}

// (the backtrace walker is a template shared with ps_sweep.hip: ps_dev.h, bt_walk)
__global__ __launch_bounds__(256) void k_backtrace(BatchD b) {
    const JobD& J = b.jobs[blockIdx.x];
    SkewCodes src;
    src.flg = b.flg + J.mat_off[0]; src.P = J.P; src.sti = 0;
    bt_walk(J, src);
}

// ref_like[i-1] = score of the cell level i was recorded from (cpp/Alignment.cpp:610-618); grid (ceil(maxn/256), njobs)
__global__ __launch_bounds__(256) void k_fill_like(BatchD b) {
    const JobD& J = b.jobs[blockIdx.y];
    if (J.out->inert) return;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= J.n0) return;
    const long long w = ((const long long*)J.rl)[t];
    if (w == 0) return;   // level not on the path: ref_like stays 0
    const int i = t + 1, j = (int)(w >> 4);   // record = column << 4 | step code << 1 | matrix (bt_walk)
    const double2 v = (b.rec + J.mat_off[0])[(int64_t)(i + j) * J.P + slot_of(i, J.P)];
    J.rl[t] = (w & 1) ? v.y : v.x;
}

// latch the reference's "stripe_width == 0" decision (cpp/Alignment.cpp:51-59) for this API call
__global__ void k_begin(BatchD b) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j == 0) *b.maxw = 0;
    if (j >= b.njobs) return;
    JobOut* O = b.jobs[j].out;
    O->inert = (b.jobs[j].force_inert || !O->has_index) ? 1 : 0;
    O->best = 0.0; O->bi = 0; O->bj = 0;
}

// out[job] = JobOut.best of every job of the batch (the results live in their AlignData's own slabs: gathered here so that one copy
// returns them)
__global__ void k_gather_best(BatchD b, double* __restrict__ out) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < b.njobs) out[j] = b.jobs[j].out->best;
}

// =================================================================================================
// launchers
// =================================================================================================
int launch_updaterefs(Runtime* rt, const BatchD& b) {
    if (!b.njobs) return PS_OK;
    hipLaunchKernelGGL(k_updaterefs, dim3(b.njobs), dim3(256), 0, rt->stream, b);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

int launch_lb(Runtime* rt, const BatchD& b, int which, int maxlbn) {
    if (!b.njobs) return PS_OK;
    if (maxlbn <= 0) return fail(PS_ERR_BAD_ARG, "launch_lb: size");
    hipLaunchKernelGGL(k_lb, dim3((maxlbn + 255) / 256, b.njobs), dim3(256), 0, rt->stream, b, which);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

int launch_lo(Runtime* rt, const BatchD& b, int ndir, int64_t maxS) {
    if (!b.njobs) return PS_OK;
    hipLaunchKernelGGL(k_lo, dim3((unsigned)((maxS + LO_PAD + 255) / 256), b.njobs * ndir), dim3(256), 0, rt->stream, b, ndir);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

constexpr int PAIR_MIN_SWEEPS = 160;
// LDS of one k_fill workgroup: the event's model rows + per half two exchange buffers, the column-maxima ring, the slow-body bitmap
static int fill_ring_cols(int P) { return P + 96 <= 512 ? 512 : (P + 96 <= 1024 ? 1024 : 2048); }
static int fill_slow_words(int64_t maxS) { return (int)((maxS + 2 * FB) / FB / 32 + 2); }
static int fill_half_bytes(int P, int64_t maxS) {
    return (int)((((size_t)2 * P * 24 + (size_t)fill_ring_cols(P) * 8 + (size_t)fill_slow_words(maxS) * 4) + 63) / 64 * 64);
}
// compact layout (lone sweeps): 64 KB of model rows, exchange records sized for the widest direction present
static int fill_compact_bytes(int P, int ndir) { return 64 * NS + 2 * P * (ndir == 2 ? 24 : 16) + fill_ring_cols(P) * 8; }
constexpr int LDS_HALF_CU = 80 * 1024;

template <int MAXT, bool PAIR, bool CMP>
static void fill_launch(Runtime* rt, const BatchD& b, const int* d_pairs, int nwg, int ndir, int P, int64_t maxS, size_t lds) {
    const dim3 grid(nwg), block(PAIR ? 2 * P : P);
    const int rc = fill_ring_cols(P), sw = fill_slow_words(maxS), hb = fill_half_bytes(P, maxS);
    with_fastdiv(b.fastdiv, [&](auto fd) { hipLaunchKernelGGL((k_fill<MAXT, PAIR, fd.value, CMP>), grid, block, lds, rt->stream, b, d_pairs, ndir, P, rc, sw, hb); });
}

int launch_fill(Runtime* rt, const BatchD& b, const std::vector<JobD>& jobs, int ndir, int64_t maxS, int P, int64_t ncols) {
    if (!b.njobs) return PS_OK;
    static std::atomic<bool> attr_set(false);   // more than the default 64 KB of dynamic LDS needs the attribute (idempotent: racing threads set the same value)
    if (!attr_set.load(std::memory_order_acquire)) {
#define PS_FILL_ATTR(...) PS_HIP(hipFuncSetAttribute((const void*)k_fill<__VA_ARGS__>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024))
        PS_FILL_ATTR(768, true, true, false); PS_FILL_ATTR(768, true, false, false);
        PS_FILL_ATTR(512, false, true, false); PS_FILL_ATTR(512, false, false, false);
        PS_FILL_ATTR(512, false, true, true); PS_FILL_ATTR(512, false, false, true);
        PS_FILL_ATTR(1024, false, true, false); PS_FILL_ATTR(1024, false, false, false);
#undef PS_FILL_ATTR
        attr_set.store(true, std::memory_order_release);
    }
    PS_HIP(hipMemsetAsync(b.cmax, 0, ncols * sizeof(double), rt->stream));
    if (P > 1024) {   // footprint wider than one lane per row: the two-slots-per-thread sweep
        static std::atomic<bool> wide_attr(false);
        if (!wide_attr.load(std::memory_order_acquire)) {
            PS_HIP(hipFuncSetAttribute((const void*)k_fill_wide<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            PS_HIP(hipFuncSetAttribute((const void*)k_fill_wide<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            wide_attr.store(true, std::memory_order_release);
        }
        const int rc = 4096;
        const size_t lds = (size_t)2 * P * 24 + (size_t)rc * 8;
        prof_begin(rt);
        with_fastdiv(b.fastdiv, [&](auto fd) { hipLaunchKernelGGL(k_fill_wide<fd.value>, dim3(b.njobs * ndir), dim3(P / 2), lds, rt->stream, b, ndir, rc); });
        PS_LAUNCH_CHECK();
        prof_end(rt, "fill", 0.0);
        if (rt->prof_on) { rt->prof["fill_wide"].launches++; if (!b.fastdiv) rt->prof["fill_ieee"].launches++; }   // (which form ran: host-side counts, no event pair)
        hipLaunchKernelGGL(k_prefix, dim3(b.njobs * ndir), dim3(64), 0, rt->stream, b, ndir);
        PS_LAUNCH_CHECK();
        return PS_OK;
    }
    // workgroups: two sweeps over the same event share one (model table in LDS): forward + backward of a job, or two
    // forward-only jobs of one event (candidate sequences of FindMutations), longest with longest
    // (a launch that fits the chip with one sweep per workgroup keeps them apart: a lone sweep finishes ~20 % sooner than a pair,
    //  and a launch this small is on some region's critical path)
    // (a test hook that tests/test_hip_parity.py changes between calls of one process: read per launch; nothing in the library or
    //  its drivers calls setenv, so the read does not race)
    const char* pm_env = getenv("PORESEQ_DEBUG_PAIR_MIN");
    const int pair_min = pm_env ? atoi(pm_env) : PAIR_MIN_SWEEPS;
    bool pair = 2 * P <= 768 && b.njobs * ndir > pair_min;
    std::vector<int> pr;
    if (pair && ndir == 2) {
        for (int j = 0; j < b.njobs; j++) { pr.push_back(2 * j); pr.push_back(2 * j + 1); }
    } else if (pair) {
        std::map<const double*, std::vector<int>> by_event;
        for (int j = 0; j < b.njobs; j++) by_event[jobs[j].model8].push_back(j);
        bool any = false;
        for (auto& kv : by_event) any |= kv.second.size() > 1;
        if (!any) pair = false;   // every event appears once (forward sweeps of many regions): nothing to share a table with
        for (auto& kv : by_event) {
            if (!pair) break;
            std::vector<int>& v = kv.second;
            std::sort(v.begin(), v.end(), [&](int x, int y) { return jobs[x].S != jobs[y].S ? jobs[x].S > jobs[y].S : x < y; });
            for (size_t k = 0; k < v.size(); k += 2) { pr.push_back(v[k]); pr.push_back(k + 1 < v.size() ? v[k + 1] : -1); }
        }
    }
    if (!pair)
        for (int jd = 0; jd < b.njobs * ndir; jd++) { pr.push_back(jd); pr.push_back(-1); }
    const int nwg = (int)pr.size() / 2;
    PS_TRY(rt->buf("fill_pairs").ensure(pr.size() * sizeof(int)));
    int* d_pairs = rt->buf("fill_pairs").as<int>();
    PS_TRY(rt->up(d_pairs, pr.data(), pr.size() * sizeof(int)));
    // a lone sweep of up to four waves takes the compact layout: two workgroups per CU (one wave of each per SIMD; measured
    // 1.5x the sweeps per second of one workgroup per CU at P = 192).  Wider ones stay alone on their CU whatever the LDS says:
    // five or six waves put two on SIMD 0, and a second workgroup's two more do not fit there beside them at 200 VGPRs
    // (tried at 168 VGPRs and exactly 80 KB for P = 384: no co-residency, and 10 % slower for the spills).
    const bool compact = !pair && P <= 256 && fill_compact_bytes(P, ndir) <= LDS_HALF_CU;
    const size_t lds = compact ? fill_compact_bytes(P, ndir) : FILL_MODEL_BYTES + (size_t)(pair ? 2 : 1) * fill_half_bytes(P, maxS);
    if (lds > 160 * 1024) return fail(PS_ERR_UNSUPPORTED, "alignment too long for the fill kernel's LDS bitmap");
    prof_begin(rt);
    if (pair) fill_launch<768, true, false>(rt, b, d_pairs, nwg, ndir, P, maxS, lds);
    else if (compact) fill_launch<512, false, true>(rt, b, d_pairs, nwg, ndir, P, maxS, lds);
    else if (P <= 512) fill_launch<512, false, false>(rt, b, d_pairs, nwg, ndir, P, maxS, lds);
    else fill_launch<1024, false, false>(rt, b, d_pairs, nwg, ndir, P, maxS, lds);
    PS_LAUNCH_CHECK();
    prof_end(rt, "fill", 0.0);
    if (rt->prof_on) {   // (which form ran: host-side counts, no event pair; fill_ieee beside the form: the launch divided)
        rt->prof[pair ? (ndir == 2 ? "fill_pair" : "fill_pair_fwd") : compact ? "fill_cmp" : P <= 512 ? "fill_512" : "fill_1024"].launches++;
        if (!b.fastdiv) rt->prof["fill_ieee"].launches++;
    }
    hipLaunchKernelGGL(k_prefix, dim3(b.njobs * ndir), dim3(64), 0, rt->stream, b, ndir);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

int launch_prefix(Runtime* rt, const BatchD& b, int ndir) {
    if (!b.njobs) return PS_OK;
    hipLaunchKernelGGL(k_prefix, dim3(b.njobs * ndir), dim3(64), 0, rt->stream, b, ndir);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

int launch_backtrace(Runtime* rt, const BatchD& b, int maxn, const MoveRun& moves) {
    if (!b.njobs) return PS_OK;
    hipLaunchKernelGGL(k_backtrace, dim3(b.njobs), dim3(256), 0, rt->stream, b);
    PS_LAUNCH_CHECK();
    PS_TRY(launch_move_stats(rt, moves));   // (reads the walk's records: before k_fill_like turns them into scores)
    if (maxn > 0) {
        hipLaunchKernelGGL(k_fill_like, dim3((maxn + 255) / 256, b.njobs), dim3(256), 0, rt->stream, b);
        PS_LAUNCH_CHECK();
    }
    return PS_OK;
}

int launch_gather_best(Runtime* rt, const BatchD& b, double* out) {
    if (!b.njobs) return PS_OK;
    hipLaunchKernelGGL(k_gather_best, dim3((b.njobs + 255) / 256), dim3(256), 0, rt->stream, b, out);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

int launch_begin(Runtime* rt, const BatchD& b) {
    if (!b.njobs) return PS_OK;
    hipLaunchKernelGGL(k_begin, dim3((b.njobs + 63) / 64), dim3(64), 0, rt->stream, b);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

}  // namespace ps
