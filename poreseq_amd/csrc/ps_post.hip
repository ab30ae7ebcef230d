// ps_post.hip — ps_posterior_stats: the sum over all alignments in an event's band (sum-product over the forward fill's lattice)
// and the expected number of each move under it.  The definition is in include/poreseq_hip.h and, in numpy,
// util.posterior_from_emissions; the recursion is fillColumn's (cpp/Alignment.cpp:189-267) with every max replaced by log-sum-exp.
//
// FP64, log domain.  One workgroup of P lanes per event, one lane per band row of the current anti-diagonal: the plain form of
// k_fill_wide (ps_kernels.hip) on k_fill's skewed layout REC[s][slot], s = i + j, slot = i mod P, with the LO / HI tables of k_lo.
// The rows in band on anti-diagonal s are lo(s) .. hi(s), all of them; a lane's row is the one row == slot (mod P) in
// [lo(s), lo(s) + P), so a row keeps its lane for as long as it is in band (P >= the widest footprint).  Whether a neighbour exists is
// decided from lo / hi of the neighbouring anti-diagonals alone, never from what a register, the exchange or memory holds: an
// out-of-band neighbour is a constant, not a load — which is also why P needs no idle slot beyond the footprint.
//   (i, j-1)    in band  <=>  lo(s-1) <= i <= hi(s-1)                       the lane's own previous value
//   (i-1, j)    in band  <=>  lo(s-1) <= i-1            (i > i0(j))         the lane one slot up, previous anti-diagonal (exchange)
//   (i-1, j-1)  read as Mp(i-1)  <=>  (i, j-1) and (i-1, j-1) both in band  (p0 < i <= p1), what the lane read one step earlier
// Column 0 is the blank column (rows 0 .. n0, all 0).  A column without a 5-mer state holds the constants M = S = 0: nothing flows
// through it and its cells are not part of logz.
//   k_post_fwd   anti-diagonals ascending; {M, S} of every band cell to REC (16 bytes per cell), a running log-sum of M per ROW in
//                the registers of the lane that owns the row, flushed when the row leaves the band; one thread reduces the rows
//                to logz in row order.
//   k_post_bwd   anti-diagonals descending; beta lives in registers and the exchange only.  At every cell the six edges INTO it are
//                weighted exp(F(pred) + w + beta - logz), F(pred) from REC (three coalesced 16-byte loads per cell); per row sums
//                in the owning lane's registers, flushed with the row's emit / col sums, then one thread per count adds the rows
//                in row order.  No floating-point atomics, and no sum whose order depends on P (which is the widest footprint of
//                the whole BATCH): a result depends neither on scheduling nor on what else is in the batch.
// Emissions are ps_dev.h's in the IEEE-division form, so one build serves every AlignData.
#include "ps_internal.h"
#include "ps_dev.h"

namespace ps {

namespace {

constexpr int POST_MAX_P = POST_MAX_SLOTS;

struct PostCtx {
    const int* __restrict__ LO;
    const int* __restrict__ HI;
    const double4* __restrict__ levs;
    const int* __restrict__ st;
    const char* __restrict__ model;
    double lsk, lst, lex, lin, off, log2pi;
    int P, S, C, n0;
};

__device__ __forceinline__ PostCtx post_ctx(const BatchD& b, const JobD& J) {
    PostCtx c;
    c.LO = b.lo + J.lo_off[0]; c.HI = b.hi + J.lo_off[0];
    c.levs = (const double4*)J.lev[0]; c.st = J.st; c.model = (const char*)J.model8;
    c.lsk = J.lsk; c.lst = J.lst; c.lex = J.lex; c.lin = J.lin; c.off = J.lik_offset; c.log2pi = b.log2pi;
    c.P = J.P; c.S = (int)J.S; c.C = J.C; c.n0 = J.n0;
    return c;
}

// the lane's row on an anti-diagonal whose lowest in-band row is lo (>= 1): the row == slot (mod P) in [lo, lo + P)
__device__ __forceinline__ int post_row(int slot, int lo, int P) {
    int d = (slot - lo) % P;
    if (d < 0) d += P;
    return lo + d;
}

__device__ __forceinline__ bool in_rows(int i, int lo, int hi) { return lo >= 0 && i >= lo && i <= hi; }

// the emission of cell (i, j) of a column whose state is `state` (>= 0)
__device__ __forceinline__ double post_emission(const PostCtx& c, int state, int i) {
    const double2* q = (const double2*)(c.model + (size_t)state * MODEL_ROW_BYTES);
    const double2 q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
    const double m[8] = {q0.x, q0.y, q1.x, q1.y, q2.x, q2.y, q3.x, q3.y};
    const double4 l4 = c.levs[i - 1];
    const double lev[4] = {l4.x, l4.y, l4.z, l4.w};
    return emission8<false>(m, lev, c.log2pi, c.off);
}

// log(exp(a) + exp(b) + ...) over N terms of which at least one is finite; -infinity stands for an absent term
template <int N>
__device__ __forceinline__ double lse(const double (&t)[N]) {
    double m = t[0];
#pragma unroll
    for (int k = 1; k < N; k++) m = fmax(m, t[k]);
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < N; k++) s += exp(t[k] - m);
    return m + log(s);
}

// a running log-sum as (maximum, sum of exp(x - maximum)); empty: (-infinity, 0)
__device__ __forceinline__ void lse_push(double& mx, double& sum, double x) {
    if (x > mx) { sum = sum * exp(mx - x) + 1.0; mx = x; }   // (exp(-infinity) = 0 for the first value)
    else sum += exp(x - mx);
}
// (mx, sum) with the running log-sum (amx, asum) appended; an empty one changes nothing
__device__ __forceinline__ void lse_merge(double& mx, double& sum, double amx, double asum) {
    if (asum == 0.0) return;
    if (amx > mx) { sum = sum * exp(mx - amx) + asum; mx = amx; }
    else sum += asum * exp(amx - mx);
}
constexpr int ROW_Z = 6;   // PostJob.row: per level 8 doubles — the six move sums of k_post_bwd, then k_post_fwd's running log-sum

}  // namespace

__global__ __launch_bounds__(POST_MAX_P) void k_post_fwd(BatchD b, const PostJob* __restrict__ pj, ps_event_posterior* __restrict__ out) {
    const JobD& J = b.jobs[blockIdx.x];
    const int tid = threadIdx.x;
    ps_event_posterior* O = out + blockIdx.x;
    if (J.out->inert || J.n0 <= 0 || J.C <= 0) {
        if (tid == 0) {
            ps_event_posterior z;
            z.n_levels = J.n0; z.inert = 1; z.n_cols = 0; z.pad = 0; z.n_cells = 0;
            z.logz = 0.0; z.e_skip = z.e_match = z.e_ignore = z.e_insert = z.e_stay = z.e_extend = 0.0;
            *O = z;
        }
        return;
    }
    const PostCtx c = post_ctx(b, J);
    const int P = c.P, slot = tid;
    const double NINF = -__builtin_inf();
    double2* __restrict__ rec = b.rec + J.mat_off[0];
    __shared__ double2 xch[2][POST_MAX_P];      // {M, S} of the lane's cell on the previous anti-diagonal
    __shared__ int r_cells[POST_MAX_P], r_cols[POST_MAX_P];
    double* __restrict__ rows = pj[blockIdx.x].row;
    xch[0][tid] = xch[1][tid] = make_double2(0.0, 0.0);
    for (int t = tid; t < c.n0; t += P) { rows[(size_t)t * 8 + ROW_Z] = NINF; rows[(size_t)t * 8 + ROW_Z + 1] = 0.0; }
    __syncthreads();
    int own = 0;                                // the row whose running log-sum the lane holds
    double cm = 0.0, dm = 0.0;                  // M of (i, j-1), and what the exchange gave one step earlier: M of (i-1, j-1)
    bool cdead = false;                         // column j-1 of the lane's previous cell has no state
    double zmx = NINF, zsum = 0.0;
    int ncell = 0, ncol = 0;
    int lo1 = -1, hi1 = -1, lo2 = -1, hi2 = -1; // lo / hi of s-1 and s-2
    for (int s = 2; s < c.S; s++) {
        const int lo = c.LO[s], hi = c.HI[s];
        const int par = s & 1;
        const int up_slot = slot == 0 ? P - 1 : slot - 1;
        const double2 up = xch[par ^ 1][up_slot];
        double nm = 0.0, ns = 0.0;
        bool dead = false;
        if (lo >= 1) {
            const int i = post_row(slot, lo, P);
            if (i <= hi) {
                const int j = s - i;
                const int state = c.st[j - 1];
                dead = state < 0;
                if (!dead) {
                    const double o = post_emission(c, state, i);
                    const bool first = j == 1;
                    const bool left = first || in_rows(i, lo1, hi1);
                    const bool diag = first || (left && in_rows(i - 1, lo2, hi2));
                    const bool upok = in_rows(i - 1, lo1, hi1);
                    const double L = (left && !first && !cdead) ? cm : 0.0;          // Mp(i), the implicit or constant 0
                    const double D = (diag && !first && !cdead) ? dm : 0.0;          // Mp(i-1)
                    if (upok) { const double t[3] = {0.0, up.x + o + c.lst, up.y + o + c.lex}; ns = lse(t); }
                    else ns = NINF;
                    const double t[6] = {0.0, L + c.lsk, D + o, diag ? D + c.lin : NINF, upok ? up.x + c.lin : NINF, ns};
                    nm = lse(t);
                    if (own != i) {            // (a row is this lane's alone: read, merge and write need no atomic)
                        if (own > 0) { double* r = rows + (size_t)(own - 1) * 8 + ROW_Z; lse_merge(r[0], r[1], zmx, zsum); }
                        own = i; zmx = NINF; zsum = 0.0;
                    }
                    lse_push(zmx, zsum, nm);
                    ncell++;
                    ncol += upok ? 0 : 1;                                            // the first row of its column's band
                }
                rec[(int64_t)s * P + slot] = make_double2(nm, ns);
            }
        }
        dm = up.x; cm = nm; cdead = dead;
        xch[par][slot] = make_double2(nm, ns);
        lo2 = lo1; hi2 = hi1; lo1 = lo; hi1 = hi;
        __syncthreads();
    }
    if (own > 0) { double* r = rows + (size_t)(own - 1) * 8 + ROW_Z; lse_merge(r[0], r[1], zmx, zsum); }
    r_cells[tid] = ncell; r_cols[tid] = ncol;
    __syncthreads();
    if (tid == 0) {
        double mx = NINF, sum = 0.0;
        long long cells = 0;
        int cols = 0;
        for (int k = 0; k < P; k++) { cells += r_cells[k]; cols += r_cols[k]; }
        for (int t = 0; t < c.n0; t++) lse_merge(mx, sum, rows[(size_t)t * 8 + ROW_Z], rows[(size_t)t * 8 + ROW_Z + 1]);   // rows in order: the same sum whatever P is
        ps_event_posterior z;
        z.n_levels = J.n0; z.inert = 0; z.n_cols = cols; z.pad = 0; z.n_cells = cells;
        z.logz = cells ? mx + log(sum) : 0.0;
        z.e_skip = z.e_match = z.e_ignore = z.e_insert = z.e_stay = z.e_extend = 0.0;
        *O = z;
    }
}

__global__ __launch_bounds__(POST_MAX_P) void k_post_bwd(BatchD b, const PostJob* __restrict__ pj, ps_event_posterior* __restrict__ out) {
    const JobD& J = b.jobs[blockIdx.x];
    const int tid = threadIdx.x;
    ps_event_posterior* O = out + blockIdx.x;
    if (J.out->inert || J.n0 <= 0 || J.C <= 0) return;       // (k_post_fwd wrote the zero record)
    const PostCtx c = post_ctx(b, J);
    const int P = c.P, slot = tid;
    const double NINF = -__builtin_inf();
    const double logz = O->logz;
    const double2* __restrict__ rec = b.rec + J.mat_off[0];
    double* __restrict__ emit = pj[blockIdx.x].emit;
    double* __restrict__ colv = pj[blockIdx.x].col;
    double* __restrict__ rows = pj[blockIdx.x].row;
    for (int t = tid; t < c.n0; t += P) {
        for (int k = 0; k < ROW_Z; k++) rows[(size_t)t * 8 + k] = 0.0;
        if (emit) { emit[t] = 0.0; colv[t] = 0.0; }
    }
    // what the lane's cell offers the cells it can be reached from: {beta_M, beta_M + obs, beta_S + obs}; -infinity: nothing
    __shared__ double xsh[6][POST_MAX_P];
    double (*xa)[POST_MAX_P] = xsh, (*xb)[POST_MAX_P] = xsh + 2, (*xs)[POST_MAX_P] = xsh + 4;
    xa[0][tid] = xb[0][tid] = xs[0][tid] = NINF;              // (the buffer the first step reads)
    xa[1][tid] = xb[1][tid] = xs[1][tid] = NINF;
    double own_bm = NINF;                                     // beta_M of (i, j+1)
    double da = NINF, db = NINF;                              // of (i+1, j+1): what the exchange gave one step earlier
    double e_skip = 0.0, e_match = 0.0, e_ign = 0.0, e_ins = 0.0, e_stay = 0.0, e_ext = 0.0;
    double em = 0.0, ec = 0.0;                                // the sums of the row the lane owns
    int own = 0;
    int lo1 = -1, hi1 = -1, lo2 = -1, hi2 = -1;               // lo / hi of s+1 and s+2
    __syncthreads();
    for (int s = c.S - 1; s >= 2; s--) {
        const int lo = c.LO[s], hi = c.HI[s];
        const int lom = c.LO[s - 1], him = c.HI[s - 1], lom2 = c.LO[s - 2], him2 = c.HI[s - 2];
        const int par = s & 1;
        const int dn_slot = slot == P - 1 ? 0 : slot + 1;
        const double na = xa[par ^ 1][dn_slot], nb = xb[par ^ 1][dn_slot], nsv = xs[par ^ 1][dn_slot];
        double pa = NINF, pb = NINF, ps_ = NINF, bm = NINF;
        if (lo >= 1) {
            const int i = post_row(slot, lo, P);
            if (i <= hi) {
                const int j = s - i;
                const int state = c.st[j - 1];
                if (state >= 0) {
                    const double o = post_emission(c, state, i);
                    const bool below = in_rows(i + 1, lo1, hi1);                   // (i+1, j) in band: i+1 <= i1(j)
                    const bool right = in_rows(i, lo1, hi1);                       // (i, j+1) in band
                    const bool dgn = below && in_rows(i + 1, lo2, hi2);            // (i+1, j+1) in band and reads this cell as Mp
                    // beta: the end, skip to (i, j+1), match and ignore to (i+1, j+1), insert and stay to (i+1, j); an offer of
                    // -infinity (a column without a state) adds nothing
                    const double t[6] = {0.0, right ? own_bm + c.lsk : NINF, dgn ? db : NINF, dgn ? da + c.lin : NINF,
                                         below ? na + c.lin : NINF, below ? nsv + c.lst : NINF};
                    bm = lse(t);
                    const double u[2] = {bm, below ? nsv + c.lex : NINF};
                    const double bs = lse(u);
                    pa = bm; pb = bm + o; ps_ = bs + o;
                    // the edges into this cell
                    const bool first = j == 1;
                    const bool left = first || in_rows(i, lom, him);
                    const bool diag = first || (left && in_rows(i - 1, lom2, him2));
                    const bool upok = in_rows(i - 1, lom, him);
                    const bool pdead = first || c.st[j - 2] < 0;
                    double L = 0.0, D = 0.0;
                    if (left && !pdead) L = rec[(int64_t)(s - 1) * P + slot].x;
                    const int up_slot = slot == 0 ? P - 1 : slot - 1;
                    if (diag && !pdead) D = rec[(int64_t)(s - 2) * P + up_slot].x;
                    if (own != i) {            // (a row is this lane's alone: its sums need no atomic)
                        if (own > 0) {
                            double* r = rows + (size_t)(own - 1) * 8;
                            r[0] += e_skip; r[1] += e_match; r[2] += e_ign; r[3] += e_ins; r[4] += e_stay; r[5] += e_ext;
                            if (emit) { emit[own - 1] += em; colv[own - 1] += ec; }
                        }
                        own = i; em = 0.0; ec = 0.0;
                        e_skip = e_match = e_ign = e_ins = e_stay = e_ext = 0.0;
                    }
                    const double wm = bm - logz, ws = bs - logz;
                    e_skip += exp(L + c.lsk + wm);
                    double w = exp(D + o + wm);
                    e_match += w;
                    if (diag) e_ign += exp(D + c.lin + wm);
                    if (upok) {
                        const double2 U = rec[(int64_t)(s - 1) * P + up_slot];
                        e_ins += exp(U.x + c.lin + wm);
                        const double w1 = exp(U.x + o + c.lst + ws), w2 = exp(U.y + o + c.lex + ws);
                        e_stay += w1; e_ext += w2;
                        w += w1; w += w2;
                    }
                    em += w; ec += w * (double)j;
                }
            }
        }
        da = na; db = nb; own_bm = bm;
        xa[par][slot] = pa; xb[par][slot] = pb; xs[par][slot] = ps_;
        lo2 = lo1; hi2 = hi1; lo1 = lo; hi1 = hi;
        __syncthreads();
    }
    if (own > 0) {
        double* r = rows + (size_t)(own - 1) * 8;
        r[0] += e_skip; r[1] += e_match; r[2] += e_ign; r[3] += e_ins; r[4] += e_stay; r[5] += e_ext;
        if (emit) { emit[own - 1] += em; colv[own - 1] += ec; }
    }
    __syncthreads();
    if (tid < ROW_Z) {
        double t = 0.0;
        for (int k = 0; k < c.n0; k++) t += rows[(size_t)k * 8 + tid];   // rows in order: the same sum whatever P is
        double* dst = tid == 0 ? &O->e_skip : tid == 1 ? &O->e_match : tid == 2 ? &O->e_ignore : tid == 3 ? &O->e_insert : tid == 4 ? &O->e_stay : &O->e_extend;
        *dst = t;
    }
    if (emit) {
        // (every row was added to by its own lane alone, in program order; the barrier above orders those adds before this pass)
        const double nan = __builtin_nan("");
        for (int t = tid; t < c.n0; t += P) { const double e = emit[t]; colv[t] = e > 0.0 ? colv[t] / e : nan; }
    }
}

int launch_post(Runtime* rt, const BatchD& b, int P, const PostJob* d_jobs, ps_event_posterior* d_out, double cells) {
    if (!b.njobs) return PS_OK;
    if (P < 64 || P > POST_MAX_P || P % 64) return fail(PS_ERR_BAD_ARG, "launch_post: slots");
    prof_begin(rt);
    hipLaunchKernelGGL(k_post_fwd, dim3(b.njobs), dim3(P), 0, rt->stream, b, d_jobs, d_out);
    PS_LAUNCH_CHECK();
    prof_end(rt, "post_fwd", 16.0 * cells);
    prof_begin(rt);
    hipLaunchKernelGGL(k_post_bwd, dim3(b.njobs), dim3(P), 0, rt->stream, b, d_jobs, d_out);
    PS_LAUNCH_CHECK();
    prof_end(rt, "post_bwd", 48.0 * cells);
    return PS_OK;
}

}  // namespace ps
