// ps_stats.hip — ps_align_stats, ps_kmer_stats and ps_move_stats.  ps_align_stats: the census of an event's ref_align array and the sufficient statistics of a shift / scale refit
// of its model, reduced on the device (include/poreseq_hip.h has the definition of a record; this file follows it line by line).
//
//   k_align_stats   grid (events of the largest AlignData, AlignData), 256 threads per event, as the reductions of ps_edit.hip
//
// The levels are read coalesced in tiles of 256.  What the census needs of a level — the column of the previous ALIGNED level and
// whether that level repeated its own predecessor — is "the last two aligned columns in front of it", and those come from a scan:
// a run of levels is summarised by a Tail (how many aligned levels it holds, capped at two, and the columns of its last two), two
// runs are joined by keeping the last two of both, which is associative.  A tile is scanned within each wavefront by cross-lane
// moves (six steps over 64 lanes), the four wavefronts meet through LDS, and the tile's Tail is carried to the next.  No level
// ever looks back over the array: a run of -1 levels costs what any other run costs.
// Accumulators live in registers and are never indexed by a runtime value.  Sums: thread t adds the qualifying levels t, t + 256,
// ... in ascending order into partials that start at +0.0, and one thread per sum then adds the 256 partials in t order — the
// order the header defines, which a host can replay bit for bit.  Counts are integers and are reduced in any order.
//
//   k_kmer_stats    grid (KMER_BLOCKS x groups of the region with the most, AlignData), 256 threads: ps_kmer_stats' tables
//
// A histogram whose bins hold floating-point sums with a DEFINED order of the adds (per (group, k-mer): events in event order,
// levels ascending, serial), so no atomics and no tree.  A workgroup owns one (region, group, block of 256 k-mers) and thread t one
// k-mer of the block; its six accumulators live in registers.  The workgroup streams the group's events in order in tiles of
// KMER_TILE levels.  Load step: thread t takes the levels t, t + 256 of the tile (coalesced), qualifies them by the n_fit rule,
// looks the state up and — only for a state of this workgroup's block — gathers the four model values, does the three divisions
// once and stores the state id and z, u, p to LDS (id -1 otherwise).  Scan step, after a barrier: every thread walks the tile's ids
// in level order, four per 16-byte LDS read and four such reads in flight (all lanes read the same address: a broadcast, no bank
// conflict; the walk is bound by LDS latency), and on a match adds
// that level's terms from LDS to its registers; a second barrier before the next tile overwrites the stage.
// Choice: KMER_BLOCKS = 4 blocks of 256 k-mers (the levels are staged four times, but a lone region with two groups puts eight
// workgroups on the chip instead of two, and each does a quarter of the divisions), KMER_TILE = 512: LDS 512 x (4 + 3 x 8) =
// 14 336 bytes per workgroup, so LDS (160 KiB per CU) admits more workgroups per CU than the four the guides advise to plan
// for; a larger tile would only save barriers (two per 512 walk steps already).
//
//   k_move_stats    grid (events of the largest AlignData, AlignData), 256 threads per event: ps_move_stats' records
//
// Runs between the backtrace walker and the kernel that turns the walker's records into ref_like (launch_backtrace, sweep_run),
// and reads those records: per recorded level column << 4 | step code << 1 | matrix, in ref_like's slot, 0 for a level not on
// the path (bt_walk, ps_dev.h, clears every level first), and in the job's result record the cell the walk started from (bi, bj)
// and the one it stopped on (term_i, term_w).  One pass over 8 bytes per level in coalesced tiles of 256; only the levels in
// (term_i, bi] are read.  A level classifies its own step; the L_SKIP steps are not recorded and are counted from the columns:
// above the record of level i the walk skipped from where the record of level i + 1 left it — that record comes from the next
// lane by a cross-lane move (the last lane of a wavefront loads it: one more 8-byte load per 64 levels, from a line its
// neighbours just fetched), for the top level it is the start cell — and the lowest recorded level adds the skips down to the
// cell the walk stopped on.  So no tile carries anything to the next and the tile loop has no barrier.  Counts are integers and
// max_skip a maximum, reduced in any order: registers, then the wavefront, then four LDS words per count.
#include "ps_dev.h"

namespace ps {

static_assert(sizeof(ps_event_moves) == 64, "ps_event_moves has no padding");
static_assert(sizeof(ps_event_stats) == 112, "ps_event_stats has no padding");
static_assert(sizeof(ps_kmer_cell) == 48, "ps_kmer_cell has no padding");
static_assert(KMER_BLOCKS * 256 == NS && KMER_TILE % 256 == 0 && KMER_TILE % 16 == 0, "a thread per k-mer, the walk takes sixteen ids per step");

namespace {

struct Tail { int n, c1, c2; };   // aligned levels in the run (0, 1, 2 = two or more); column of the last, of the one before it

__device__ inline Tail tail_join(const Tail a, const Tail b) {   // the run a followed by the run b
    Tail r;
    r.n = b.n == 0 ? a.n : (b.n == 1 ? min(a.n + 1, 2) : 2);
    r.c1 = b.n ? b.c1 : a.c1;
    r.c2 = b.n == 2 ? b.c2 : (b.n == 1 ? a.c1 : a.c2);
    return r;
}
__device__ inline Tail tail_up(const Tail x, int d) {   // lane l gets the Tail of lane l - d of its wavefront (lanes below d: their own)
    Tail r;
    r.n = __shfl_up(x.n, d, 64); r.c1 = __shfl_up(x.c1, d, 64); r.c2 = __shfl_up(x.c2, d, 64);
    return r;
}
__device__ inline int wave_sum(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ inline long long wave_sum(long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

constexpr int ST_NCNT = 10;   // n_aligned, n_insert, n_unaligned, n_step, n_stay, n_extend, n_jump, n_back, n_nostate, n_fit

__global__ __launch_bounds__(256) void k_align_stats(const StatJob* __restrict__ J, const StatRegion* __restrict__ R, ps_event_stats* __restrict__ out) {
    const StatRegion rg = R[blockIdx.y];
    if ((int)blockIdx.x >= rg.njobs) return;   // (the same for every thread of the block)
    const StatJob j = J[rg.job0 + blockIdx.x];
    __shared__ int s_tail[4][3];
    __shared__ double s_sum[6][256];
    __shared__ int s_cnt[ST_NCNT][4];
    __shared__ long long s_gap[4];
    __shared__ int s_first;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    if (t == 0) s_first = 0;
    Tail carry = {0, 0, 0};   // of all tiles so far; every thread keeps its own copy
    int n_al = 0, n_ins = 0, n_un = 0, n_step = 0, n_stay = 0, n_ext = 0, n_jump = 0, n_back = 0, n_nost = 0, n_fit = 0;
    long long gap = 0;
    double sw = 0.0, swm = 0.0, swmm = 0.0, swr = 0.0, swmr = 0.0, swrr = 0.0;
    for (int base = 0; base < j.n; base += 256) {
        const int i = base + t;
        const bool in = i < j.n;
        const double ra = in ? j.ra[i] : 0.0;
        const double mean = in ? j.mean[i] : 0.0;
        const bool al = ra > 0.0;
        const int c = al ? (int)fmin(ra, 2147483647.0) : 0;
        // inclusive scan of the tile's Tails within the wavefront, then the Tail of everything in front of this level
        Tail inc = {al ? 1 : 0, c, 0};
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const Tail o = tail_up(inc, d);
            if (lane >= d) inc = tail_join(o, inc);
        }
        if (lane == 63) { s_tail[w][0] = inc.n; s_tail[w][1] = inc.c1; s_tail[w][2] = inc.c2; }
        Tail pre = tail_up(inc, 1);
        if (lane == 0) pre = Tail{0, 0, 0};
        __syncthreads();
        Tail front = carry;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const Tail wk = {s_tail[k][0], s_tail[k][1], s_tail[k][2]};
            if (k < w) front = tail_join(front, wk);
            carry = tail_join(carry, wk);
        }
        pre = tail_join(front, pre);
        __syncthreads();   // (s_tail is written again by the next tile)
        if (!in) continue;
        if (!al) { if (ra < 0.0) n_ins++; else n_un++; continue; }
        n_al++;
        if (pre.n == 0) s_first = c;   // (one level of the event: a single writer)
        else {
            const int d = c - pre.c1;   // both in 0 .. 2^31 - 1
            const bool prev_rep = pre.n == 2 && pre.c1 == pre.c2;
            if (d == 0) { if (prev_rep) n_ext++; else n_stay++; }
            else if (d == 1) n_step++;
            else if (d > 1) { n_jump++; gap += d - 1; }
            else n_back++;
        }
        const int k = (c >= 1 && c <= j.S) ? j.st[c - 1] : -1;
        if (k < 0 || k >= NS) { n_nost++; continue; }
        n_fit++;
        const double mk = j.model[k], sk = j.model[NS + k];
        const double wt = 1.0 / (sk * sk), wm = wt * mk, r = mean - mk;
        sw += wt; swm += wm; swmm += wm * mk; swr += wt * r; swmr += wm * r; swrr += (wt * r) * r;
    }
    s_sum[0][t] = sw; s_sum[1][t] = swm; s_sum[2][t] = swmm; s_sum[3][t] = swr; s_sum[4][t] = swmr; s_sum[5][t] = swrr;
    {
        const int c0 = wave_sum(n_al), c1 = wave_sum(n_ins), c2 = wave_sum(n_un), c3 = wave_sum(n_step), c4 = wave_sum(n_stay);
        const int c5 = wave_sum(n_ext), c6 = wave_sum(n_jump), c7 = wave_sum(n_back), c8 = wave_sum(n_nost), c9 = wave_sum(n_fit);
        const long long g = wave_sum(gap);
        if (lane == 0) {
            s_cnt[0][w] = c0; s_cnt[1][w] = c1; s_cnt[2][w] = c2; s_cnt[3][w] = c3; s_cnt[4][w] = c4;
            s_cnt[5][w] = c5; s_cnt[6][w] = c6; s_cnt[7][w] = c7; s_cnt[8][w] = c8; s_cnt[9][w] = c9;
            s_gap[w] = g;
        }
    }
    __syncthreads();
    ps_event_stats* o = out + rg.job0 + blockIdx.x;
    if (t < 6) {   // one thread per sum, partials in t order
        double sum = 0.0;
        for (int l = 0; l < 256; l++) sum += s_sum[t][l];
        double* dst = &o->sw;   // sw, swm, swmm, swr, swmr, swrr lie in this order
        dst[t] = sum;
    } else if (t == 64) {
        auto cnt = [&](int k) { return s_cnt[k][0] + s_cnt[k][1] + s_cnt[k][2] + s_cnt[k][3]; };
        o->n_levels = j.n; o->n_aligned = cnt(0); o->n_insert = cnt(1); o->n_unaligned = cnt(2);
        o->n_step = cnt(3); o->n_stay = cnt(4); o->n_extend = cnt(5); o->n_jump = cnt(6); o->n_back = cnt(7);
        o->n_nostate = cnt(8); o->n_fit = cnt(9);
        o->first_col = carry.n ? s_first : 0; o->last_col = carry.n ? carry.c1 : 0; o->reserved = 0;
        o->n_gap_cols = s_gap[0] + s_gap[1] + s_gap[2] + s_gap[3];
    }
}

__global__ __launch_bounds__(256) void k_kmer_stats(const StatJob* __restrict__ J, const StatRegion* __restrict__ R, ps_kmer_cell* __restrict__ out) {
    const StatRegion rg = R[blockIdx.y];
    const int g = (int)blockIdx.x / KMER_BLOCKS, kb = (int)blockIdx.x % KMER_BLOCKS;
    if (g >= rg.ngroups) return;   // (the same for every thread of the block)
    __shared__ __attribute__((aligned(16))) int s_k[KMER_TILE];
    __shared__ double s_z[KMER_TILE], s_u[KMER_TILE], s_p[KMER_TILE];
    const int t = threadIdx.x, mine = kb * 256 + t;
    long long n = 0;
    double sz = 0.0, szz = 0.0, sp = 0.0, spu = 0.0, spv = 0.0;
    for (int q = 0; q < rg.njobs; q++) {
        const StatJob j = J[rg.job0 + q];
        if (j.grp != g) continue;   // (uniform: the barriers below are met by all threads or by none)
        for (int base = 0; base < j.n; base += KMER_TILE) {
            const int m = min(KMER_TILE, j.n - base);
#pragma unroll
            for (int l = t; l < KMER_TILE; l += 256) {
                int k = -1;
                if (l < m) {
                    const double ra = j.ra[base + l];
                    if (ra > 0.0) {
                        const int c = (int)fmin(ra, 2147483647.0);
                        if (c >= 1 && c <= j.S) k = j.st[c - 1];
                    }
                    if (k < 0 || k >= NS || (k >> 8) != kb) k = -1;
                }
                if (k >= 0) {
                    const double mk = j.model[k], sk = j.model[NS + k], mu = j.model[3 * NS + k], lam = j.model[4 * NS + k];
                    s_z[l] = (j.mean[base + l] - mk) / sk;
                    s_u[l] = j.stdv[base + l] / mu;
                    s_p[l] = lam / mu;
                }
                s_k[l] = k;
            }
            __syncthreads();
            auto take = [&](int l) {
                const double z = s_z[l], u = s_u[l], p = s_p[l];
                n++; sz += z; szz += z * z; sp += p; spu += p * u; spv += p / u;
            };
            for (int l = 0; l < m; l += 16) {   // (ids behind m are -1 up to the end of the tile; four reads in flight: the walk is LDS latency)
                const int4* ids = reinterpret_cast<const int4*>(&s_k[l]);
                const int4 a = ids[0], b = ids[1], c = ids[2], d = ids[3];
                if (a.x == mine) take(l);
                if (a.y == mine) take(l + 1);
                if (a.z == mine) take(l + 2);
                if (a.w == mine) take(l + 3);
                if (b.x == mine) take(l + 4);
                if (b.y == mine) take(l + 5);
                if (b.z == mine) take(l + 6);
                if (b.w == mine) take(l + 7);
                if (c.x == mine) take(l + 8);
                if (c.y == mine) take(l + 9);
                if (c.z == mine) take(l + 10);
                if (c.w == mine) take(l + 11);
                if (d.x == mine) take(l + 12);
                if (d.y == mine) take(l + 13);
                if (d.z == mine) take(l + 14);
                if (d.w == mine) take(l + 15);
            }
            __syncthreads();   // (the stage is written again by the next tile)
        }
    }
    ps_kmer_cell* o = out + ((size_t)(rg.tab0 + g) * NS + mine);
    o->n = n; o->sz = sz; o->szz = szz; o->sp = sp; o->spu = spu; o->spv = spv;
}

constexpr int MV_NCNT = 7;   // n_match, n_ignore, n_insert, n_stay, n_extend, n_skip_runs, max_skip

__device__ inline int wave_max(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
    return v;
}
// columns the step recorded in `w` moves to the left: 1 for MATCH / IGNORE, 0 for INSERT / STAY / EXTEND
__device__ inline int move_dj(long long w) {
    const unsigned st = (unsigned)(w >> 1) & 7u;
    return (st == M_MATCH || st == M_IGNORE) ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_move_stats(const MoveJob* __restrict__ J, const StatRegion* __restrict__ R, ps_event_moves* __restrict__ out) {
    const StatRegion rg = R[blockIdx.y];
    if ((int)blockIdx.x >= rg.njobs) return;   // (the same for every thread of the block)
    const MoveJob j = J[rg.job0 + blockIdx.x];
    const JobOut O = *j.out;
    __shared__ int s_cnt[MV_NCNT][4];
    __shared__ long long s_cols[4];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    // inert: the walker left at once (refs and records untouched, term_i / term_w stale); no positive score: it walked nothing
    const bool walked = !O.inert && O.bi > 0;
    const int top = walked ? min(O.bi, j.n) : 0, bj = walked ? O.bj : 0;
    const int low = walked ? clampi(O.term_i, 0, top) : 0;   // levels low + 1 .. top were recorded
    const int low_col = walked ? (O.term_w >> 3) : 0;
    int n_m = 0, n_ig = 0, n_in = 0, n_st = 0, n_ex = 0, n_run = 0, mx = 0;
    long long cols = 0;
    // (with the per-level arrays every level is visited, since the levels off the path get their zeros here)
    const bool per_level = j.step || j.col;
    const int first = per_level ? 0 : (low / 256) * 256, last = per_level ? j.n : top;
    for (int base = first; base < last; base += 256) {
        const int i = base + t + 1;   // the level, 1-based
        const bool on = i > low && i <= top;
        const long long rec = on ? j.rec[i - 1] : 0ll;
        // the record of level i + 1: the next lane's, or — last lane of the wavefront — loaded
        long long up = (lane == 63 && on && i < top) ? j.rec[i] : 0ll;
        const long long nxt = __shfl_down(rec, 1, 64);
        if (lane != 63) up = nxt;
        const int st = (int)(rec >> 1) & 7, c = (int)(rec >> 4);
        if (i <= j.n) {
            if (j.step) j.step[i - 1] = (uint8_t)st;
            if (j.col) j.col[i - 1] = c;
        }
        if (!on) continue;
        n_m += st == (int)M_MATCH; n_ig += st == (int)M_IGNORE; n_in += st == (int)M_INSERT;
        n_st += st == (int)M_STAY; n_ex += st == (int)M_EXTEND;
        const int above = (i == top ? bj : (int)(up >> 4) - move_dj(up)) - c;
        const int below = i == low + 1 ? (c - move_dj(rec)) - low_col : 0;
        n_run += (above > 0) + (below > 0);
        mx = max(mx, max(above, below));
        cols += above + below;
    }
    {
        const int c0 = wave_sum(n_m), c1 = wave_sum(n_ig), c2 = wave_sum(n_in), c3 = wave_sum(n_st), c4 = wave_sum(n_ex), c5 = wave_sum(n_run);
        const int c6 = wave_max(mx);
        const long long g = wave_sum(cols);
        if (lane == 0) {
            s_cnt[0][w] = c0; s_cnt[1][w] = c1; s_cnt[2][w] = c2; s_cnt[3][w] = c3; s_cnt[4][w] = c4; s_cnt[5][w] = c5; s_cnt[6][w] = c6;
            s_cols[w] = g;
        }
    }
    __syncthreads();
    if (t == 0) {
        auto cnt = [&](int k) { return s_cnt[k][0] + s_cnt[k][1] + s_cnt[k][2] + s_cnt[k][3]; };
        ps_event_moves m;
        m.n_levels = j.n; m.inert = O.inert ? 1 : 0;
        m.top_level = top; m.top_col = bj;
        m.low_level = top > low ? low + 1 : 0; m.low_col = low_col;
        m.end_kind = walked ? (O.term_w & 1) : 0;
        m.n_match = cnt(0); m.n_ignore = cnt(1); m.n_insert = cnt(2); m.n_stay = cnt(3); m.n_extend = cnt(4);
        m.n_skip_runs = cnt(5);
        m.max_skip = max(max(s_cnt[6][0], s_cnt[6][1]), max(s_cnt[6][2], s_cnt[6][3]));
        m.n_skip_cols = s_cols[0] + s_cols[1] + s_cols[2] + s_cols[3];
        out[rg.job0 + blockIdx.x] = m;
    }
}

}  // namespace

int launch_move_stats(Runtime* rt, const MoveRun& mv) {
    if (!mv.jobs || mv.nregs <= 0 || mv.maxE <= 0) return PS_OK;
    prof_begin(rt);
    hipLaunchKernelGGL(k_move_stats, dim3(mv.maxE, mv.nregs), dim3(256), 0, rt->stream, mv.jobs, mv.regs, mv.out);
    PS_LAUNCH_CHECK();
    prof_end(rt, "move_stats", mv.alg_bytes);
    return PS_OK;
}

int launch_kmer_stats(Runtime* rt, const StatJob* d_jobs, const StatRegion* d_regs, int nregs, int maxG, double alg_bytes, ps_kmer_cell* d_out) {
    if (nregs <= 0 || maxG <= 0) return PS_OK;
    prof_begin(rt);
    hipLaunchKernelGGL(k_kmer_stats, dim3(KMER_BLOCKS * maxG, nregs), dim3(256), 0, rt->stream, d_jobs, d_regs, d_out);
    PS_LAUNCH_CHECK();
    prof_end(rt, "kmer_stats", alg_bytes);
    return PS_OK;
}

int launch_align_stats(Runtime* rt, const StatJob* d_jobs, const StatRegion* d_regs, int nregs, int maxE, double alg_bytes, ps_event_stats* d_out) {
    if (nregs <= 0 || maxE <= 0) return PS_OK;
    prof_begin(rt);
    hipLaunchKernelGGL(k_align_stats, dim3(maxE, nregs), dim3(256), 0, rt->stream, d_jobs, d_regs, d_out);
    PS_LAUNCH_CHECK();
    prof_end(rt, "align_stats", alg_bytes);
    return PS_OK;
}

}  // namespace ps
