// ps_sw.hip — full-matrix Smith-Waterman (swfull, cpp/swlib.cpp:211-340) on gfx950.
//
// Integer DP, +5 / -4 / -8 (linear gaps), bit-exact with the reference including its tie rules (left with >,
// then up with >, then diagonal with >=, floor 0; the first strict maximum in column-major order starts the
// traceback; the traceback stops at the first score <= 0).
//
// Formulation.  With a linear gap cost the row recurrence  H(i,j) = max(c(i,j), H(i,j-1) - 8),
// c(i,j) = max(0, H(i-1,j-1) + s, H(i-1,j) - 8)  is a prefix maximum:  H(i,j) + 8j = max_{j'<=j} (c(i,j') + 8j').
// So a whole row is computed at once — every c from the previous row, then one max-scan across the lanes (DPP) —
// with no systolic skew: all 64 lanes work on every row.
//
// Layout.  Lane l of wave w owns K consecutive columns (K = 4, 8 or 16: sw_launch, ps_swhost.cpp); 8 waves x
// 64 lanes x K columns = one "super-strip" = one 512-thread workgroup, and a pair takes as many super-strips as
// its columns need, all in the same launch and pipelined over rows like the waves inside one (a 10 kb pair runs
// on five CUs at K = 4, on three at K = 8).  The waves form a pipeline over rows: in
// pipeline step s wave w does rows 8(s-w)+1 .. 8(s-w)+8 and hands the H values of its last column to wave
// w+1 through LDS (one workgroup barrier per 8 rows).  Nothing per cell goes to memory: the fill keeps only
//   rowsave  H(64q, *)    every 64th row       (top boundaries of 64-row blocks)
//   colsave  H(*, 64c)    every 64th column    (left boundaries of 64-column blocks)
//   blkmax   max H per (row block, wave strip)
// and the traceback kernel recomputes the 64 x 64 tiles its path crosses (the same row routine with one column
// per lane, this time deriving the 4-bit step codes into LDS) — about 300 of the 25 000 tiles of a 10 kb pair.
// The starting cell is located by recomputing only the strips whose block maximum equals the global maximum.
//
// Band mode (SwPair::wb > 0, the packed fill only).  Strips of 512 columns, one wave each, four waves per pair; strip s computes only its
// rows [512 s + 1 - wb, 512 s + 512 + wb] (whole 64-row blocks), every cell outside them counts as 0.  That region holds the band
// |i - j| <= wb, so the banded value Hb is a lower bound of the true H*, and any path the region misses leaves the band, with at most
// min(i, j) matches and at least wb + 1 - |i - j| gap steps:  H* <= max(Hb, B),  B(i, j) = 5 min(i, j) - 8 max(0, wb + 1 - |i - j|).
// So a cell with Hb >= B is exact.  The result is certified by the traceback kernel: the banded maximum must exceed
// U = max B over all cells (then it is the true maximum and its first cell the reference's), and every cell the walk reads (the path
// cell and its left, upper and diagonal neighbours) must pass Hb >= B.  A pair that fails is redone on the full matrix (sw_finish).
#include "ps_dev.h"
#include "ps_sw.h"

namespace ps {

// geometry constants, SwPair, the result record's names and the address of every checkpoint entry: ps_swplan.h

// inclusive prefix maximum over the 64 lanes of a wave: six v_max_i32 with a DPP-shifted first operand; a lane without a source
// (the first lanes of a row for row_shr, the rows a row_mask leaves out) is disabled for that instruction and keeps its value.
// Written out: through __builtin_amdgcn_update_dpp the compiler emits v_mov + v_mov_dpp + v_max per step (18 instead of 6 vector
// instructions per row: a sixth of the fill's).  The two wait states a DPP read needs after the write of its source are the s_nop 1.
__device__ __forceinline__ int wave_scan_max(int v) {
    asm("s_nop 1\n\tv_max_i32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\tv_max_i32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\tv_max_i32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\tv_max_i32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\tv_max_i32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
        "s_nop 1\n\tv_max_i32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf"
        : "+v"(v));
    return v;
}

// One row of one wave's strip, in shifted form: the lane's k-th column is carried as G[k] = H + 8k, which turns
// the in-lane part of the prefix maximum into a plain running max and folds the gap steps into constants
// (7 integer instructions per cell).  G[] holds row i-1 on entry and row i on return.
//   c1     character of row i (wave-uniform)          bl     H(i, first column - 1)   (left boundary, uniform)
//   bprev  H(i-1, first column - 1) (uniform)         lane   lane index, lane0 = lane ? -2^29 : 0
//   c2[] and c1 hold characters shifted left by 4
// MODE 0: values only.  MODE 1: also track the column-major first cell equal to `target` in (fc, fr).
// MODE 2 (K == 1): also return the cell's step code  step | 4*(score > 0) | 8*(characters equal) | 16*(exact), where exact means
// that the cell and the three neighbours its step compares pass the band certificate Hb >= B (target = wb; always set when wb = 0).
template <int K, int MODE>
__device__ __forceinline__ unsigned sw_row(int (&G)[K], const int (&c2)[K], const int c1, const int bl, const int bprev,
                                           const int lane, const int lane0, const int target, const int i, const int jfirst, int& fc, int& fr) {
    // H(i-1, j-1) of this lane's first column: the previous row's last column of the lane to the left (+ 8(K-1))
    const int d0 = __builtin_amdgcn_update_dpp(bprev + 8 * (K - 1), G[K - 1], 0x138 /*wave_shr:1*/, 0xf, 0xf, false);
    int y[K];
    int sd0 = 0, up0 = 0;
#pragma unroll
    for (int k = 0; k < K; k++) {
        // substitution penalty without a compare / select (VALU -> SGPR -> v_cndmask round trips are slow on
        // gfx950): characters are held shifted left by 4, so c2 ^ c1 is 0 when equal and >= 16 otherwise
        const int pen = min(c2[k] ^ c1, 9);
        // diagonal + substitution score, and value above - 8, both shifted by 8k
        const int sd = (k ? G[k - 1] + 13 : d0 + (5 - 8 * (K - 1))) - pen;
        const int up = G[k] - 8;
        if (k == 0) { sd0 = sd; up0 = up; }
        y[k] = max(max(sd, up), 8 * k);
    }
    // running maximum over the lane's columns as a two-level tree (groups of 4): depth 6 instead of K - 1
    constexpr int NG = (K + 3) / 4;
    int tg[NG];
#pragma unroll
    for (int g = 0; g < NG; g++) {
#pragma unroll
        for (int k = 4 * g + 1; k < min(4 * g + 4, K); k++) y[k] = max(y[k], y[k - 1]);
        const int last = y[min(4 * g + 3, K - 1)];
        tg[g] = g ? max(last, tg[g - 1]) : last;
    }
    // scan of the lanes' last columns (as H + 8K*lane); the left boundary enters through lane 0
    int z = tg[NG - 1] + (8 * K * lane - 8 * (K - 1));
    z = max(z, (bl - 8 * K) + lane0);   // lane0 = 0 in lane 0, -2^29 elsewhere
    z = wave_scan_max(z);
    // H(i, first column - 1) of this lane, minus one gap
    const int hl8 = __builtin_amdgcn_update_dpp(bl - 8 * K, z, 0x138, 0xf, 0xf, false) + (8 * K - 8 * K * lane - 8);
    unsigned code = 0;
#pragma unroll
    for (int k = 0; k < K; k++) {
        const int gn = k >= 4 ? max(max(y[k], tg[k / 4 - 1]), hl8) : max(y[k], hl8);
        if (MODE == 2 && k == 0) {
            // reference order (cpp/swlib.cpp:243-263): left with >, up with >, diagonal with >=
            const int l0 = max(hl8, 0), m = max(l0, up0);
            const unsigned step = sd0 >= m ? 3u : (up0 > l0 ? 2u : (hl8 > 0 ? 1u : 0u));
            code = step | (gn > 0 ? 4u : 0u) | (c2[0] == c1 ? 8u : 0u);
            const int j = jfirst + 1;
            if (!target || (gn >= band_bound(i, j, target) && hl8 + 8 >= band_bound(i, j - 1, target) &&
                            up0 + 8 >= band_bound(i - 1, j, target) && d0 >= band_bound(i - 1, j - 1, target)))
                code |= 16u;
        }
        if (MODE == 1) {
            const int col = jfirst + k + 1;
            if (gn == target + 8 * k && col < fc) { fc = col; fr = i; }
        }
        G[k] = gn;
    }
    return code;
}

// ---- fill: grid (super-strips, pairs), block 64 * SWW ------------------------------------------------------------------
// The workgroups of one pair's super-strips run concurrently, as one more level of the row pipeline: the last wave
// of strip ss stores its boundary column (colsave) and, every 64 rows, publishes the row count with an agent-scope
// release; the first wave of strip ss+1 acquires it before it reads those rows.  A workgroup takes its strip index from a
// per-pair ticket (not from blockIdx, whose dispatch order HIP does not promise): whoever waits for strip ss-1 knows that a
// workgroup holding that ticket started before it, so the producer is always resident or finished.
//
// One workgroup per pair (WW = 16 waves, K = 8 / 16 columns per lane: up to 8 192 / 16 384 columns): the whole pair is
// ONE super-strip, its sixteen waves pipeline over rows through LDS and nobody waits on another workgroup — no boundary column in
// global memory, no tickets, no spinning waves holding slots and registers while their producer is scheduled.  Built for the round-3
// review's item 5, parity-tested, and slower than the chained strips where it was meant to win (see sw_launch, ps_swhost.cpp): selected only by
// PORESEQ_SW_FORM=one.
constexpr int SW_SPIN_LIMIT = 1 << 22;
// byte code of the columns past n2 that fill out a lane's span: above every byte, so that no byte of seq1 — a NUL least of all — matches
// the padding (its shifted form, SW_PAD << 4, still fits the packed fill's 16-bit halves)
constexpr int SW_PAD = 256;
template <int K, int WW>
__global__ __launch_bounds__(64 * WW) void k_sw_fill(const SwPair* pairs, const char* chars, int* rowsave, int* colsave,
                                                  int* blkmax, int* prog, int* ticket, int* res) {
    __shared__ int s_ticket;
    if (threadIdx.x == 0) s_ticket = atomicAdd(&ticket[blockIdx.y], 1);
    __syncthreads();
    const int ss = s_ticket;
    const SwPair p = pairs[blockIdx.y];
    if (p.n1 <= 0 || p.n2 <= 0 || ss * WW * 64 * K >= p.n2) return;
    int* prog_my = prog + (int64_t)blockIdx.y * gridDim.x + ss;
    const bool has_next = (ss + 1) * WW * 64 * K < p.n2;   // strip ss+1 exists: it consumes this strip's last column
    int seen = 0;                                           // rows of strip ss-1 known to be complete
    const int t = threadIdx.x, w = t >> 6, l = t & 63;
    const int gw = ss * WW + w;
    const int wfirst = gw * 64 * K;            // 0-based first column of the wave
    const bool wave_on = wfirst < p.n2;
    const int jbase = wfirst + l * K;
    const char* s1 = chars + p.s1_off;
    const char* s2 = chars + p.s2_off;
    int c2[K], G[K], bmk[K];
#pragma unroll
    for (int k = 0; k < K; k++) { c2[k] = (jbase + k < p.n2 ? (int)(unsigned char)s2[jbase + k] : SW_PAD) << 4; G[k] = 8 * k; bmk[k] = 0; }
    const int lane0 = l ? -(1 << 29) : 0;
    __shared__ int hand[WW][2][SWB];
    // this lane's last column is column jbase + K (1-based); every 64th column is kept as a tile boundary
    const bool keeps = ((jbase + K) & 63) == 0 && jbase + K <= p.n2;
    int* csave = col_base<false>(colsave, p, (jbase + K) >> 6, SwWin{0});
    const int* cprev = col_base<false>(colsave, p, wfirst >> 6, SwWin{0});   // H(*, wfirst): used by wave 0 when ss > 0
    if (wave_on && keeps) csave[0] = 0;
    int bprev = 0, dummy_c = 0, dummy_r = 0;
    const int nchunks = (p.n1 + SWB - 1) / SWB;
    // row characters (and, for the first wave of a later super-strip, the left boundary) are fetched one chunk
    // ahead; the workgroup barrier waits for LDS only, so global loads and stores stay in flight across it
    auto fetch = [&](int c, int& ch, int& bd) {
        ch = 1; bd = 0;
        const int i0 = c * SWB;
        if (w == 0 && ss > 0 && c >= 0 && c < nchunks) {   // wave-uniform: the rows of this chunk must have been published
            const int need = min(p.n1, (i0 + SWB + 63) & ~63);
            int spins = 0;
            for (; seen < need && spins < SW_SPIN_LIMIT; spins++) {
                seen = __hip_atomic_load(prog_my - 1, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
                if (seen < need) __builtin_amdgcn_s_sleep(8);
            }
            if (seen < need && l == 0) atomicOr(sw_record(res, p) + SWR_TIMED_OUT, 1);   // gave up waiting: the pair's result is not valid
        }
        if (wave_on && c >= 0 && c < nchunks && l < SWB && i0 + l < p.n1) {
            ch = (int)(unsigned char)s1[i0 + l] << 4;
            if (w == 0 && gw > 0) bd = cprev[i0 + 1 + l];
        }
    };
    int ch_nx, bd_nx;
    fetch(0 - w, ch_nx, bd_nx);
    for (int s = 0; s < nchunks + WW - 1; s++) {
        const int c = s - w;
        const int ch1 = ch_nx, bd1 = bd_nx;
        fetch(c + 1, ch_nx, bd_nx);
        if (wave_on && c >= 0 && c < nchunks) {
            const int i0 = c * SWB;
            int bnd = bd1;
            if (w > 0 && l < SWB && i0 + l < p.n1) bnd = hand[w - 1][(s - 1) & 1][l];
            int hl[SWB];
#pragma unroll
            for (int r = 0; r < SWB; r++) hl[r] = 0;
#pragma unroll
            for (int r = 0; r < SWB; r++) {
                if (i0 + r < p.n1) {
                    const int bl = __builtin_amdgcn_readlane(bnd, r), c1 = __builtin_amdgcn_readlane(ch1, r);
                    sw_row<K, 0>(G, c2, c1, bl, bprev, l, lane0, 0, 0, 0, dummy_c, dummy_r);
                    bprev = bl;
#pragma unroll
                    for (int k = 0; k < K; k++) bmk[k] = max(bmk[k], G[k]);
                    const int hlast = G[K - 1] - 8 * (K - 1);
                    if (l == 63) hand[w][s & 1][r] = hlast;
                    hl[r] = hlast;
                }
            }
            // the kept boundary column's rows of this chunk in two 16-byte stores (round 6: one 4-byte store per row and kept column was
            // 101 G of a bench step's 225 G L1 -> L2 write requests, profiles/r06_mem.json)
            if (keeps) {
                if (i0 + SWB <= p.n1) {
                    *(v4i_a4*)(csave + i0 + 1) = (v4i_a4){hl[0], hl[1], hl[2], hl[3]};
                    *(v4i_a4*)(csave + i0 + 5) = (v4i_a4){hl[4], hl[5], hl[6], hl[7]};
                } else {
#pragma unroll
                    for (int r = 0; r < SWB; r++) if (i0 + r < p.n1) csave[i0 + r + 1] = hl[r];
                }
            }
            const int iend = min(i0 + SWB, p.n1);
            if ((iend & 63) == 0 || iend == p.n1) {   // row block q complete
                const int q = (iend - 1) >> 6;
                int bm = 0;
#pragma unroll
                for (int k = 0; k < K; k++) { bm = max(bm, bmk[k] - 8 * k); bmk[k] = 0; }
                for (int o = 32; o; o >>= 1) bm = max(bm, __shfl_xor(bm, o));
                if (l == 0) blkmax[bm_index<false>(p, q, gw, SwWin{0})] = bm;
                // lane 63 of the strip's last wave stored the boundary column of these rows: release them to strip ss+1
                if (has_next && w == WW - 1 && l == 63) __hip_atomic_store(prog_my, iend, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                if (iend < p.n1) {                    // row 64(q+1) is the top boundary of block q+1
                    int* rs = rowsave + rs_index<false>(p, q + 1, jbase, ss);
#pragma unroll
                    for (int k = 0; k < K; k++) if (jbase + k < p.n2) rs[k] = G[k] - 8 * k;
                }
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
}

// ---- packed fill: two columns per 32-bit register --------------------------------------------------------------------
// Scores are at most 5 x min(n1, n2): for pairs up to 13 000 bases they fit 16 bits, and gfx950's packed 16-bit integer instructions
// (v_pk_add / sub / min / max_u16, with op_sel picking halves) work on two columns at once.  A lane owns 8 columns in four
// registers; column k is carried as G' = H + 8 (k + 1) (unsigned: the diagonal entering the lane's first column, H + 0, stays >= 0).
// Same recurrence, same saved rows / columns / block maxima as k_sw_fill<8, 8> — the traceback kernel reads either — at ~6.6 vector
// instructions per cell instead of ~10: the substitution term costs one LDS load per row when the row's base is A / C / G / T (per-lane
// tables of 13 / 4 for the four bases in LDS; any other byte takes xor / min / sub).
typedef unsigned short us2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ us2 pk_of(unsigned v) { return __builtin_bit_cast(us2, v); }
__device__ __forceinline__ unsigned un_pk(us2 v) { return __builtin_bit_cast(unsigned, v); }

// one row; P[m] = G' of columns 2m (low half) and 2m + 1 (high half): row i - 1 on entry, row i on return.  sp[m]: 13 where the
// column's base equals the row's, 4 elsewhere (both halves).  bl / bprev: H(i, first column - 1) / H(i - 1, first column - 1) of the wave.
__device__ __forceinline__ void sw_row_pk(unsigned (&P)[4], const unsigned (&sp)[4], const int bl, const int bprev, const int lane8k, const int lane0) {
    // H(i-1, lane's first column - 1): the left lane's last column of the previous row (G' = H + 8 K there)
    const int plast = (int)(P[3] >> 16);
    const int d0 = __builtin_amdgcn_update_dpp(bprev + 8 * PKK, plast, 0x138 /*wave_shr:1*/, 0xf, 0xf, false) - 8 * PKK;
    us2 y[4];
#pragma unroll
    for (int m = 0; m < 4; m++) {
        // G' of the column to the left, both halves: the diagonal neighbour in the same shift (its + 8 per column is the gap step's)
        const unsigned S = m ? __builtin_amdgcn_alignbit(P[m], P[m - 1], 16) : ((P[0] << 16) | (unsigned)d0);
        const us2 sd = pk_of(S) + pk_of(sp[m]);                                               // diagonal + substitution score (+ 8: the shift)
        const us2 up = __builtin_elementwise_sub_sat(pk_of(P[m]), (us2){8, 8});                // above - 8 (+ 8 - 8 of the shift: the same column)
        const us2 fl = {(unsigned short)(8 * (2 * m + 1)), (unsigned short)(8 * (2 * m + 2))};  // the floor H = 0
        y[m] = __builtin_elementwise_max(__builtin_elementwise_max(sd, up), fl);
    }
    // running maximum over the lane's eight columns (the shift absorbs the gap steps)
#pragma unroll
    for (int m = 0; m < 4; m++) {
        const us2 lo = {y[m].x, y[m].x};
        y[m] = __builtin_elementwise_max(y[m], lo);
        if (m) { const us2 ph = {y[m - 1].y, y[m - 1].y}; y[m] = __builtin_elementwise_max(y[m], ph); }
    }
    // scan of the lanes' last columns (as H + 8 K (lane + 1)); the wave's left boundary enters through lane 0 (as a lane -1)
    int z = (int)y[3].y + lane8k;
    z = max(z, bl + lane0);                  // lane0 = 0 in lane 0, -2^29 elsewhere
    z = wave_scan_max(z);
    const int hl = __builtin_amdgcn_update_dpp(bl, z, 0x138, 0xf, 0xf, false) - lane8k;   // H(i, lane's first column - 1): reaches column k as hl in the G' shift
    const us2 hl2 = {(unsigned short)hl, (unsigned short)hl};
#pragma unroll
    for (int m = 0; m < 4; m++) P[m] = un_pk(__builtin_elementwise_max(y[m], hl2));
}

// (at most 64 registers: a wave then fits beside two 224-register sweep waves on a SIMD; the compiler takes 79 when left alone)
// BAND: one workgroup of WW waves per pair; wave w runs the pair's 512-column strips w, w + WW, ... one after the other, each over its rows
// [r0 + 1, rend] only; rows of the left neighbour's boundary column beyond its last row (pend) and the row above r0 + 1 count as 0.  A
// strip waits for its left neighbour (the previous wave) through an LDS progress word, 64 rows at a time; the neighbour starts 512 rows
// earlier and a strip spans 512 + 2 wb rows, so with WW <= 1 + 2 wb / 512 no wave waits once the pipeline is full.  Full matrix: r0 = 0,
// rend = pend = n1.  (Measured: band strips chained as one-wave workgroups through global memory, like the full fill's, made the whole
// bench 1.5x slower: strip s waits for 512 s rows, so a 10 kb pair holds twenty wave slots that mostly poll, beside the strip sweeps.
// One wave per pair over all its strips: no faster than the full fill, its launches twice as long.)
template <int WW, bool BAND>
__global__ __launch_bounds__(64 * WW) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_sw_fill_pk(const SwPair* pairs, const char* chars, int* rowsave, int* colsave,
                                                       int* blkmax, int* prog, int* ticket, int* res) {
    constexpr int K = PKK;
    static_assert(!BAND || 64 * K == SWBS, "band strips are one wave");
    constexpr int WP = BAND ? 1 : WW;   // waves in one strip's row pipeline
    constexpr int KEY = 32768;          // band progress word: strip x KEY + rows done in it (at most 64 nbb < KEY)
    __shared__ int s_ticket, s_key[WW];
    if (!BAND) {
        if (threadIdx.x == 0) s_ticket = atomicAdd(&ticket[blockIdx.y], 1);
    } else if (threadIdx.x < WW) {
        s_key[threadIdx.x] = 0;
    }
    __syncthreads();
    const SwPair p = pairs[blockIdx.y];
    const int nstrip = BAND ? (p.n2 + SWBS - 1) / SWBS : 1;
    for (int it = BAND ? (int)(threadIdx.x >> 6) : 0; it < nstrip; it += BAND ? WW : 1) {
    const int ss = BAND ? it : s_ticket;
    if (p.n1 <= 0 || p.n2 <= 0 || ss * WP * 64 * K >= p.n2) return;
    int* prog_my = prog + (int64_t)blockIdx.y * gridDim.x + ss;
    const bool has_next = !BAND && (ss + 1) * WW * 64 * K < p.n2;
    int seen = 0;
    const int t = threadIdx.x, w = t >> 6, l = t & 63, wp = BAND ? 0 : w;
    const int gw = BAND ? ss : ss * WW + w;
    const int wfirst = gw * 64 * K;
    const bool wave_on = wfirst < p.n2;
    const int jbase = wfirst + l * K;
    const char* s1 = chars + p.s1_off;
    const char* s2 = chars + p.s2_off;
    // substitution scores of the lane's eight columns against each of the four bases, in LDS: a row reads its table with one 16-byte
    // LDS load (no vector instruction per column; tables in registers picked by a uniform branch cost 17 register moves per row)
    __shared__ uint4 s_sp[4][64 * WW];
    unsigned P[4], bmk[4], c2p[4];
    {
        unsigned tb[4][4];
#pragma unroll
        for (int m = 0; m < 4; m++) {
            const unsigned a = jbase + 2 * m < p.n2 ? (unsigned)(unsigned char)s2[jbase + 2 * m] : (unsigned)SW_PAD, b = jbase + 2 * m + 1 < p.n2 ? (unsigned)(unsigned char)s2[jbase + 2 * m + 1] : (unsigned)SW_PAD;
            c2p[m] = (a << 4) | (b << 20);
            auto tab = [&](unsigned ch) { return (a == ch ? 13u : 4u) | ((b == ch ? 13u : 4u) << 16); };
            tb[0][m] = tab('A'); tb[1][m] = tab('C'); tb[2][m] = tab('G'); tb[3][m] = tab('T');
            P[m] = (unsigned)(8 * (2 * m + 1)) | ((unsigned)(8 * (2 * m + 2)) << 16);
            bmk[m] = 0u;
        }
#pragma unroll
        for (int q = 0; q < 4; q++) s_sp[q][threadIdx.x] = make_uint4(tb[q][0], tb[q][1], tb[q][2], tb[q][3]);
    }
    const int lane0 = l ? -(1 << 29) : 0, lane8k = 8 * K * l;
    __shared__ int hand[WW][2][SWB];
    const bool keeps = ((jbase + K) & 63) == 0 && jbase + K <= p.n2;
    const SwWin win = band_win<BAND>(p, ss), pwin = band_left<BAND>(win);   // the window of this strip, and of its left neighbour
    const int r0 = 64 * band_q0<BAND>(win), rend = col_hi<BAND>(p, win);
    const int pend = col_hi<BAND>(p, pwin);   // last row of the left neighbour's boundary column
    int* csave = col_base<BAND>(colsave, p, (jbase + K) >> 6, win);
    const int* cprev = col_base<BAND>(colsave, p, wfirst >> 6, pwin);
    if (wave_on && keeps) csave[r0] = 0;
    int bprev = 0;
    const int cb = r0 / SWB, ce = (rend + SWB - 1) / SWB;   // chunks of this strip
    auto fetch = [&](int c, int& ch, int& bd) {
        ch = 1; bd = 0;
        const int i0 = c * SWB;
        if (BAND && ss > 0 && c >= cb && c < ce) {      // the previous wave's strip: rows relative to its first
            const int want = (ss - 1) * KEY + min(pend, (i0 + SWB + 63) & ~63) - 64 * band_q0<BAND>(pwin);
            int spins = 0;
            for (; seen < want && spins < SW_SPIN_LIMIT; spins++) {
                seen = __hip_atomic_load(&s_key[(w + WW - 1) % WW], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (seen < want) __builtin_amdgcn_s_sleep(2);
            }
            if (seen < want && l == 0) atomicOr(sw_record(res, p) + SWR_TIMED_OUT, 1);
        }
        if (!BAND && w == 0 && ss > 0 && c >= cb && c < ce) {
            const int need = min(pend, (i0 + SWB + 63) & ~63);
            int spins = 0;
            for (; seen < need && spins < SW_SPIN_LIMIT; spins++) {
                seen = __hip_atomic_load(prog_my - 1, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
                if (seen < need) __builtin_amdgcn_s_sleep(8);
            }
            if (seen < need && l == 0) atomicOr(sw_record(res, p) + SWR_TIMED_OUT, 1);
        }
        if (wave_on && c >= cb && c < ce && l < SWB && i0 + l < rend) {
            ch = (int)(unsigned char)s1[i0 + l];
            if (wp == 0 && gw > 0 && i0 + 1 + l <= pend) bd = cprev[i0 + 1 + l];
        }
    };
    int ch_nx, bd_nx;
    fetch(cb - wp, ch_nx, bd_nx);
    if (BAND && gw > 0 && r0 > 0 && r0 <= pend) bprev = cprev[r0];   // the corner H(r0, first column - 1): published with the first chunk's rows
    for (int s = 0; s < ce - cb + WP - 1; s++) {
        const int c = cb + s - wp;
        const int ch1 = ch_nx, bd1 = bd_nx;
        fetch(c + 1, ch_nx, bd_nx);
        if (wave_on && c >= cb && c < ce) {
            const int i0 = c * SWB;
            int bnd = bd1;
            if (wp > 0 && l < SWB && i0 + l < rend) bnd = hand[w - 1][(s - 1) & 1][l];
            int hl[SWB];
#pragma unroll
            for (int r = 0; r < SWB; r++) hl[r] = 0;
#pragma unroll
            for (int r = 0; r < SWB; r++) {
                if (i0 + r < rend) {
                    const int bl = __builtin_amdgcn_readlane(bnd, r), c1 = __builtin_amdgcn_readlane(ch1, r);   // c1: the row's base (uniform)
                    const int bidx = c1 == 'A' ? 0 : c1 == 'C' ? 1 : c1 == 'G' ? 2 : c1 == 'T' ? 3 : -1;       // (scalar selects)
                    unsigned sp[4];
                    if (bidx >= 0) {
                        const uint4 v = s_sp[bidx][threadIdx.x];
                        sp[0] = v.x; sp[1] = v.y; sp[2] = v.z; sp[3] = v.w;
                    } else {
                        const unsigned c1p = ((unsigned)c1 << 4) | ((unsigned)c1 << 20);
#pragma unroll
                        for (int m = 0; m < 4; m++) sp[m] = un_pk((us2){13, 13} - __builtin_elementwise_min(pk_of(c2p[m] ^ c1p), (us2){9, 9}));
                    }
                    sw_row_pk(P, sp, bl, bprev, lane8k, lane0);
                    bprev = bl;
#pragma unroll
                    for (int m = 0; m < 4; m++) bmk[m] = un_pk(__builtin_elementwise_max(pk_of(bmk[m]), pk_of(P[m])));
                    const int hlast = (int)(P[3] >> 16) - 8 * K;
                    if (!BAND && l == 63) hand[w][s & 1][r] = hlast;
                    hl[r] = hlast;
                }
            }
            // the kept boundary column's rows of this chunk in two 16-byte stores (round 6: one 4-byte store per row and kept column was
            // 101 G of a bench step's 225 G L1 -> L2 write requests, profiles/r06_mem.json)
            if (keeps) {
                if (i0 + SWB <= rend) {
                    *(v4i_a4*)(csave + i0 + 1) = (v4i_a4){hl[0], hl[1], hl[2], hl[3]};
                    *(v4i_a4*)(csave + i0 + 5) = (v4i_a4){hl[4], hl[5], hl[6], hl[7]};
                } else {
#pragma unroll
                    for (int r = 0; r < SWB; r++) if (i0 + r < rend) csave[i0 + r + 1] = hl[r];
                }
            }
            const int iend = min(i0 + SWB, rend);
            if ((iend & 63) == 0 || iend == rend) {   // row block q complete
                const int q = (iend - 1) >> 6;
                int bm = 0;
#pragma unroll
                for (int m = 0; m < 4; m++) {
                    bm = max(bm, (int)(bmk[m] & 0xffffu) - 8 * (2 * m + 1));
                    bm = max(bm, (int)(bmk[m] >> 16) - 8 * (2 * m + 2));
                    bmk[m] = 0u;
                }
                for (int o = 32; o; o >>= 1) bm = max(bm, __shfl_xor(bm, o));
                if (l == 0) blkmax[bm_index<BAND>(p, q, gw, win)] = bm;
                if (has_next && w == WW - 1 && l == 63) __hip_atomic_store(prog_my, iend, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                if (BAND && l == 63) __hip_atomic_store(&s_key[w], ss * KEY + iend - r0, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (iend < rend) {
                    int* rs = rowsave + rs_index<BAND>(p, q + 1, jbase, ss);
#pragma unroll
                    for (int m = 0; m < 4; m++) {
                        if (jbase + 2 * m < p.n2) rs[2 * m] = (int)(P[m] & 0xffffu) - 8 * (2 * m + 1);
                        if (jbase + 2 * m + 1 < p.n2) rs[2 * m + 1] = (int)(P[m] >> 16) - 8 * (2 * m + 2);
                    }
                }
            }
        }
        if (!BAND) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
    if (BAND && l == 63) __hip_atomic_store(&s_key[w], (ss + 1) * KEY, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);   // strip done
    }
}

// recompute rows 64q+1 .. 64q+nrows of the strip of 64K columns that starts at 0-based column c0 (a multiple of 64); one wave
template <int K, int MODE>
__device__ __forceinline__ void sw_tile(const SwPair& p, const char* s1, const char* s2, const int* rowsave, const int* colsave,
                                        const int q, const int c0, const int nrows, const int l, const int target, int& fc, int& fr,
                                        unsigned char (*codes)[64]) {
    const int jbase = c0 + l * K;
    int c2[K], G[K];
    const int* rs = rowsave + rs_index(p, q, jbase);
    const bool top = q > band_q0(p, c0 / SWBS);   // (band mode: a tile never crosses a strip; the strip's top boundary is 0)
#pragma unroll
    for (int k = 0; k < K; k++) {
        const bool ok = jbase + k < p.n2;
        c2[k] = (ok ? (int)(unsigned char)s2[jbase + k] : SW_PAD) << 4;
        G[k] = ((ok && top) ? rs[k] : 0) + 8 * k;
    }
    const int* cprev = colsave + col_base(p, c0 >> 6);   // H(*, c0): rows up to chi, 0 below
    const int chi = c0 > 0 ? col_hi(p, c0 >> 6) : 0;
    int bprev = c0 > 0 && 64 * q <= chi ? cprev[64 * q] : 0;
    int bnd = 0, ch1 = 1;
    if (l < nrows) { ch1 = (int)(unsigned char)s1[64 * q + l] << 4; if (c0 > 0 && 64 * q + 1 + l <= chi) bnd = cprev[64 * q + 1 + l]; }
    const int lane0 = l ? -(1 << 29) : 0;
    for (int r = 0; r < nrows; r++) {
        const int bl = __builtin_amdgcn_readlane(bnd, r), c1 = __builtin_amdgcn_readlane(ch1, r);
        const unsigned cd = sw_row<K, MODE>(G, c2, c1, bl, bprev, l, lane0, target, 64 * q + r + 1, jbase, fc, fr);
        if (MODE == 2) codes[r][l] = (unsigned char)cd;   // MODE 2 runs with K == 1
        bprev = bl;
    }
}

// ---- locate the starting cell, then trace back; grid (pairs), block 64 ------------------------------------------
// SUMMARY: the same walk, counted instead of stored (SwForm, ps_swplan.h): nothing goes to `out` (no buffer exists), and the record gets the
// walk's ends and its gap steps next to the pair and match counts — what a caller would read off the reversed index lists.  In walk
// order the first entry is the lists' last, the last entry their first; every value below is wave-uniform.
// SW_MAP: the same walk writes part[i1] = i2 for every non-zero seq1 index of the lists (0 where the base faces a gap) into the pair's
// table of n1 + 2 ints (`out`, which stays on the device) — i1 runs down from hi to lo, every index once, all of them inside 1 .. n1 —
// and the record gets lo, hi, whether an entry with i1 == 0 exists and the i2 of the first such entry in list order (the last one the
// walk meets: overwritten as it goes): RemapRec, ps_remap.h.  Entries with i1 == 0 write nothing to the table.
template <int K, int FORM>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(K <= 8 ? 8 : 4, 8))) void k_sw_trace(const SwPair* pairs, const char* chars, const int* rowsave, const int* colsave,
                                                 const int* blkmax, int* out, int* res) {
    __shared__ unsigned char codes[64][64];
    __builtin_amdgcn_s_setprio(PS_WALKER_PRIO);   // one serial wave per pair at the end of FindMutations' chain (ps_dev.h, chain_priority)
    const SwPair p = pairs[blockIdx.x];
    const int l = threadIdx.x;
    int* o = sw_record(res, p);
    const char* s1 = chars + p.s1_off;
    const char* s2 = chars + p.s2_off;
    const int* bmx = blkmax + bm_base(p);
    int best = 0;
    if (p.n1 > 0 && p.n2 > 0)
        for (int k = l; k < bm_count(p); k += 64) best = max(best, bmx[k]);
    for (int s = 32; s; s >>= 1) best = max(best, __shfl_xor(best, s));
    if (p.wb) {   // the banded maximum is the true one only above U = max over all cells of B (out-of-band cells at |i - j| = wb + 1)
        if (best <= band_u(p.n1, p.n2, p.wb)) {
            if (l == 0) sw_rec(o, SWR_INEXACT) = 1;
            return;
        }
    }
    if (best <= 0) {
        if (l == 0) { sw_rec(o, SWR_SCORE) = 0; sw_rec(o, SWR_BI) = 0; sw_rec(o, SWR_BJ) = 0; sw_rec(o, SWR_N_PAIRS) = 0; sw_rec(o, SWR_N_MATCH) = 0; }
        return;
    }
    // first cell with the maximum in column-major order: smallest column, then smallest row
    int bi = 0, bj = 0;
    for (int gw = 0; gw < p.ngw && !bj; gw++) {
        int fc = 0x7fffffff, fr = 0x7fffffff;
        const int qa = band_q0(p, gw), qb = band_q1(p, gw);
        for (int q0 = qa; q0 < qb; q0 += 64) {
            const int q = q0 + l;
            unsigned long long hit = __ballot(q < qb && blkmax[bm_index(p, q, gw)] == best);
            while (hit) {
                const int qq = q0 + (int)__builtin_ctzll(hit);
                hit &= hit - 1;
                sw_tile<K, 1>(p, s1, s2, rowsave, colsave, qq, gw * 64 * K, min(64, p.n1 - 64 * qq), l, best, fc, fr, codes);
            }
        }
        for (int s = 32; s; s >>= 1) {
            const int oc = __shfl_xor(fc, s), orow = __shfl_xor(fr, s);
            if (oc < fc || (oc == fc && orow < fr)) { fc = oc; fr = orow; }
        }
        if (fc != 0x7fffffff) { bj = fc; bi = fr; }
    }
    constexpr bool SUMMARY = FORM == SW_SUMMARY, LISTS = FORM == SW_LISTS, MAP = FORM == SW_MAP;
    int* oi = LISTS || MAP ? out + p.out_off : nullptr;   // (map form: the partner table)
    int* oj = LISTS ? oi + (p.n1 + p.n2 + 2) : nullptr;
    int i = bi, j = bj, np = 0, nm = 0;
    int w1 = 0, w2 = 0, e1 = 0, e2 = 0, g1 = 0, g2 = 0;   // summary: first and latest entry of the walk, entries with a 0 on either side
    int mlo = 0, mhi = 0, m0 = 0, my0 = 0;                // map: RemapRec
    bool done = false, inexact = false;
    while (!done && i > 0 && j > 0) {
        const int q = (i - 1) >> 6, cb = (j - 1) >> 6;   // 64 x 64 tile holding (i, j), one column per lane
        const int r0 = 64 * q + 1, cfirst = 64 * cb + 1;
        int dc = 0, dr = 0;
        __syncthreads();
        sw_tile<1, 2>(p, s1, s2, rowsave, colsave, q, 64 * cb, i - 64 * q, l, p.wb, dc, dr, codes);
        __syncthreads();
        // lane m looks m cells ahead on the diagonal: a run of diagonal steps is emitted at once
        while (true) {
            if (!(i > 0 && j > 0)) { done = true; break; }
            if (i < r0 || j < cfirst) break;   // left the tile
            const int ii = i - l, jj = j - l;
            unsigned code = 0;
            if (ii >= r0 && jj >= cfirst) code = codes[ii - r0][jj - cfirst];
            const unsigned long long dm = __ballot((code & 7u) == 7u);   // diagonal step from a cell with score > 0
            const int run = __builtin_amdgcn_readfirstlane(dm == ~0ull ? 64 : (int)__builtin_ctzll(~dm));
            if (__ballot(l < run && !(code & 16u))) { inexact = true; done = true; break; }   // band certificate
            if (LISTS) { if (l < run) { oi[np + l] = ii; oj[np + l] = jj; } }
            else if (MAP) { if (l < run) oi[ii] = jj; if (run) { if (!mhi) mhi = i; mlo = i - run + 1; } }
            else if (run) { if (!np) { w1 = i; w2 = j; } e1 = i - run + 1; e2 = j - run + 1; }
            nm += (int)__popcll(__ballot((code & 8u) && l < run));
            np += run; i -= run; j -= run;
            if (run == 64) continue;
            if (!(i > 0 && j > 0)) { done = true; break; }
            if (i < r0 || j < cfirst) break;
            const unsigned cr = __builtin_amdgcn_readlane(code, run);
            if (!(cr & 16u)) { inexact = true; done = true; break; }
            if (!(cr & 4u)) { done = true; break; }   // score <= 0
            const unsigned stp = cr & 3u;
            if (stp == 1u) {
                if (LISTS) { if (l == 0) { oi[np] = 0; oj[np] = j; } }
                else if (MAP) { m0 = 1; my0 = j; }
                else { if (!np) { w1 = 0; w2 = j; } e1 = 0; e2 = j; g1++; }
                np++; j--;
            } else if (stp == 2u) {
                if (LISTS) { if (l == 0) { oi[np] = i; oj[np] = 0; } }
                else if (MAP) { if (l == 0) oi[i] = 0; if (!mhi) mhi = i; mlo = i; }
                else { if (!np) { w1 = i; w2 = 0; } e1 = i; e2 = 0; g2++; }
                np++; i--;
            } else { done = true; break; }
        }
    }
    auto put = [&](SwRec f, int v) { sw_rec(o, f) = v; };
    if (l == 0) { put(SWR_SCORE, best); put(SWR_BI, bi); put(SWR_BJ, bj); put(SWR_N_PAIRS, np); put(SWR_N_MATCH, nm); put(SWR_INEXACT, inexact ? 1 : 0); }
    if (SUMMARY && l == 0) { put(SWR_FIRST1, e1); put(SWR_FIRST2, e2); put(SWR_LAST1, w1); put(SWR_LAST2, w2); put(SWR_GAP1, g1); put(SWR_GAP2, g2); }
    if (MAP && l == 0) { put(SWR_MAP_LO, mlo); put(SWR_MAP_HI, mhi); put(SWR_MAP_HAS0, m0); put(SWR_MAP_Y0, my0); }
}

// the one function that names the kernels (ps_sw.h)
int sw_run(hipStream_t st, const SwDev& d, int np, int nss, int K, int waves, bool packed, bool band, SwForm form) {
#define PS_SW_TRACE(K_) (form == SW_SUMMARY ? k_sw_trace<K_, SW_SUMMARY> : (form == SW_MAP ? k_sw_trace<K_, SW_MAP> : k_sw_trace<K_, SW_LISTS>))
    auto run = [&](auto fill, dim3 grid, int wv, int* prog, int* ticket, auto trace) -> int {
        hipLaunchKernelGGL(fill, grid, dim3(64 * wv), 0, st, d.pairs, d.chars, d.row, d.col, d.blk, prog, ticket, d.res);
        PS_LAUNCH_CHECK();
        hipLaunchKernelGGL(trace, dim3(np), dim3(64), 0, st, d.pairs, d.chars, d.row, d.col, d.blk, d.out, d.res);
        PS_LAUNCH_CHECK();
        return PS_OK;
    };
    const dim3 strips(nss, np);
    // (kernels come out in the code object in the order they are first named here)
    if (packed && !band) return run(k_sw_fill_pk<SWW, false>, strips, SWW, d.prog, d.ticket, PS_SW_TRACE(8));
    if (band) return run(k_sw_fill_pk<SWBW, true>, dim3(1, np), SWBW, nullptr, nullptr, PS_SW_TRACE(8));
    switch (100 * waves + K) {
        case 100 * SWW1 + 8: return run(k_sw_fill<8, SWW1>, strips, SWW1, d.prog, d.ticket, PS_SW_TRACE(8));
        case 100 * SWW1 + 16: return run(k_sw_fill<16, SWW1>, strips, SWW1, d.prog, d.ticket, PS_SW_TRACE(16));
        case 100 * SWW + 4: return run(k_sw_fill<4, SWW>, strips, SWW, d.prog, d.ticket, PS_SW_TRACE(4));
        case 100 * SWW + 16: return run(k_sw_fill<16, SWW>, strips, SWW, d.prog, d.ticket, PS_SW_TRACE(16));
        case 100 * SWW + 8: return run(k_sw_fill<8, SWW>, strips, SWW, d.prog, d.ticket, PS_SW_TRACE(8));
    }
#undef PS_SW_TRACE
    return fail(PS_ERR_BAD_ARG, "Smith-Waterman: no fill of " + std::to_string(K) + " columns per lane on " + std::to_string(waves) + " waves is built");
}

}  // namespace ps
