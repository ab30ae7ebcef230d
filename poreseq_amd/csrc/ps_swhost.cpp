// ps_swhost.cpp — host side of the Smith-Waterman module: the band choice, one launch in stages (sw_launch), its results and the redo of
// failed band certificates (sw_finish), chunking by device memory.  The kernels and sw_run, the one function that names them, are in
// ps_sw.hip; the pair record, the result record and the checkpoint layout in ps_swplan.h.
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>

#include "ps_host.h"
#include "ps_plan.h"
#include "ps_sw.h"

namespace ps {

// -------------------------------------------------------------------------------------------------
// band choice.  PORESEQ_SW_BAND = off / auto (default) / force, PORESEQ_SW_BAND_W = half-width (a multiple of 64, default 1024); both
// read per call (test hooks).  auto bands a pair when the band computes at most half the matrix, the lengths differ by at most wb / 2
// and a k-mer sample says the alignment is close and near the diagonal (high-identity seeds pass, reads against the draft do not:
// a failed certificate costs the band fill on top of the full one).  force bands every pair the packed fill can take.
static int band_width_env() {
    const char* e = getenv("PORESEQ_SW_BAND_W");
    const int w = e ? atoi(e) : SW_BAND_W;
    return w >= 64 ? std::min(w, 8192) / 64 * 64 : SW_BAND_W;   // (8192: the fill's progress word holds 64 nbb < 32768 rows)
}

// 12-mers of s1 at ~256 evenly spaced positions, each looked up in s2 within +-32 of the diagonal offset the previous hit left (indels
// drift it); a pair is close when >= 60 % are found and no hit lies further than wb / 2 from the main diagonal (~96 % identity and up:
// a loss 5 min(n1, n2) - M below the certificate's 5 (wb + 1 - |n1 - n2|) at wb = 1024)
static bool band_close(const std::string& s1, const std::string& s2, int wb) {
    constexpr int KM = 12, WIN = 32, NS = 256;
    const int n1 = (int)s1.size(), n2 = (int)s2.size();
    if (n1 < 4 * KM || n2 < 4 * KM) return false;
    auto code = [](const std::string& x, int at) {
        uint32_t v = 0;
        for (int k = 0; k < KM; k++) v = (v << 2) | ((x[at + k] >> 1) & 3);   // A C G T -> 0 1 3 2 (other bytes: some code)
        return v;
    };
    std::vector<uint32_t> c2(n2 - KM + 1);
    {
        uint32_t v = 0;
        for (int k = 0; k < n2; k++) {
            v = ((v << 2) | ((s2[k] >> 1) & 3)) & ((1u << (2 * KM)) - 1);
            if (k >= KM - 1) c2[k - KM + 1] = v;
        }
    }
    const int step = std::max(1, (n1 - KM) / NS);
    int hits = 0, tries = 0, d = 0, dmax = 0;
    for (int p = 0; p + KM <= n1; p += step) {
        tries++;
        const uint32_t v = code(s1, p);
        int best = -1;
        for (int o = 0; o <= WIN && best < 0; o++)
            for (int sg = 0; sg < 2 && best < 0; sg++) {
                const int q = p + d + (sg ? -o : o);
                if (q >= 0 && q + KM <= n2 && c2[q] == v) best = q;
            }
        if (best >= 0) { hits++; d = best - p; dmax = std::max(dmax, std::abs(d)); }
    }
    return hits * 10 >= tries * 6 && 2 * dmax <= wb;
}

// PORESEQ_SW_PK=0 (tests): never the packed 16-bit fill
static bool packed_allowed() { const char* e = getenv("PORESEQ_SW_PK"); return !e || atoi(e) != 0; }

int sw_band_choice(const std::string& s1, const std::string& s2) {
    const char* e = getenv("PORESEQ_SW_BAND");   // (per call, as PORESEQ_SW_BAND_W and PORESEQ_SW_PK: test hooks)
    const int mode = !e || !strcmp(e, "auto") ? 1 : (!strcmp(e, "force") ? 2 : 0);
    const int n1 = (int)s1.size(), n2 = (int)s2.size();
    if (!mode || n1 <= 0 || n2 <= 0 || std::min(n1, n2) > SW_PK_MAXLEN) return 0;
    if (!packed_allowed()) return 0;   // the band fill is a form of the packed one
    const int wb = band_width_env();
    if (mode == 2) return wb;
    if (2 * std::abs(n1 - n2) > wb || band_cells(n1, n2, wb) > 0.5 * (double)n1 * n2) return 0;
    return band_close(s1, s2, wb) ? wb : 0;
}

static std::atomic<int64_t> g_band[5];   // pairs banded, fell back, maxima near a band edge, band cells, full-matrix cells

void sw_band_counters(int64_t out[5]) { for (int k = 0; k < 5; k++) out[k] = g_band[k].load(); }

// -------------------------------------------------------------------------------------------------
// sw_launch: enqueue a batch of pairwise alignments on the runtime's second stream (asynchronous), in stages
namespace {
struct Launch {
    Runtime* rt; const SwInput& in; SwJob* job; SwForm form;
    int np;
    std::vector<int> wb;                // band half-width per pair, input order
    int K = 4, WW = SWW, nss = 1;       // the full-matrix pairs' fill: columns per lane, waves per workgroup, chained strips
    int nf = 0, nb = 0;                 // full-matrix pairs, band pairs
    std::vector<SwPair> dev;            // the pairs in device order
    SwPools tot;
    size_t nprog = 0;                   // progress per strip + one ticket counter per pair (full-matrix pairs)
    SwDev dv{};
    hipStream_t st = nullptr;
    size_t res_bytes() const { return (size_t)tot.res * sizeof(int); }
};
}  // namespace

// stage 1: K columns per lane on WW waves per workgroup, chained over nss strips
static void choose_form(Launch& L) {
    int maxn2 = 1;
    for (int k = 0; k < L.np; k++) if (!L.wb[k]) maxn2 = std::max(maxn2, (int)L.in[k].second->size());
    // 4 columns per lane = 2048 per workgroup: a 10 kb pair runs as five chained workgroups, all but the last full (8 columns per
    // lane: three, the last 44 % used, 7.8 instead of 6.6 ms per pair).  8 columns per lane spread the row scan over twice the cells:
    // 17 % fewer vector instructions per pair — with several lock-step batches in flight the chip is short of vector issue, not of
    // latency, and the wide build is the faster one (bench: 189.9 against 184.5 kb/s).  PORESEQ_SW_K forces either (tests).
    L.K = live_runtimes() > 1 ? 8 : 4;
    if (const char* e = getenv("PORESEQ_SW_K")) L.K = atoi(e) == 16 ? 16 : (atoi(e) == 8 ? 8 : 4);
    // PORESEQ_SW_FORM=one: one workgroup of 16 waves per pair when the longest sequence fits 16 x 64 x K columns — no chained workgroups,
    // nothing spins.  Measured and NOT the default: in the bench (14 lock-step batches in flight) 176.9 kb/s against 190.3 with the
    // chained strips — a 10 kb pair keeps 10 of the 16 waves busy, holds a whole CU, and meets at a 16-wave barrier every eight rows.
    const char* form = getenv("PORESEQ_SW_FORM");   // (a test hook that the tests change between calls of one process: read per launch)
    const int k1 = maxn2 <= SWW1 * 64 * 8 ? 8 : (maxn2 <= SWW1 * 64 * 16 ? 16 : 0);   // (K divides 64: every 64th column is some lane's last)
    if (form && !strcmp(form, "one") && k1) { L.K = k1; L.WW = SWW1; }
    const int sswidth = L.WW * 64 * L.K;
    L.nss = (maxn2 + sswidth - 1) / sswidth;
}

// stage 2: every pair's place in the pools (input order; results by res_off) and the device order
static void lay_out(Launch& L) {
    SwJob* job = L.job;
    job->pairs.assign(L.np, SwPair());
    job->cells = 0; job->band_cells = 0;
    for (int k = 0; k < L.np; k++) {
        SwPair& p = job->pairs[k];
        sw_lay_out(p, (int)L.in[k].first->size(), (int)L.in[k].second->size(), L.wb[k], L.form, L.K, L.WW, L.tot);
        p.s1_off = (int64_t)job->pool.size(); job->pool += *L.in[k].first;
        p.s2_off = (int64_t)job->pool.size(); job->pool += *L.in[k].second;
        job->cells += (double)p.n1 * p.n2;
        job->band_cells += p.wb ? band_cells(p.n1, p.n2, p.wb) : (double)p.n1 * p.n2;
    }
    job->pool.push_back(0);
    job->out_tot = L.tot.out;
    for (int k : sw_device_order(L.wb)) L.dev.push_back(job->pairs[k]);
    L.nb = (int)std::count_if(L.wb.begin(), L.wb.end(), [](int w) { return w != 0; });
    L.nf = L.np - L.nb;
    job->nband = L.nb;
    L.nprog = (size_t)L.nf * (L.nss + 1) + 1;
}

// stage 3: buffers, uploads, memsets
static int place(Launch& L) {
    Runtime* rt = L.rt;
    const bool lists = L.form == SW_LISTS, map = L.form == SW_MAP;
    PS_TRY(rt->buf("sw_pairs").ensure(L.np * sizeof(SwPair)));
    PS_TRY(rt->buf("sw_chars").ensure(L.job->pool.size()));
    PS_TRY(rt->buf("sw_row").ensure(L.tot.row * sizeof(int)));
    PS_TRY(rt->buf("sw_col").ensure(L.tot.col * sizeof(int)));
    PS_TRY(rt->buf("sw_blk").ensure(L.tot.blk * sizeof(int)));
    PS_TRY(rt->buf("sw_prog").ensure(L.nprog * sizeof(int)));
    if (lists) PS_TRY(rt->buf("sw_out").ensure(L.tot.out * sizeof(int)));
    PS_TRY(rt->buf("sw_res").ensure(L.res_bytes()));
    SwPair* d_pairs = rt->buf("sw_pairs").as<SwPair>();
    char* d_chars = rt->buf("sw_chars").as<char>();
    int* d_prog = rt->buf("sw_prog").as<int>();
    L.dv = {d_pairs, d_chars, rt->buf("sw_row").as<int>(), rt->buf("sw_col").as<int>(), rt->buf("sw_blk").as<int>(), d_prog, d_prog + (size_t)L.nf * L.nss,
            lists ? rt->buf("sw_out").as<int>() : (map ? L.job->d_map : nullptr), rt->buf("sw_res").as<int>()};
    PS_TRY(second_stream(rt, &L.st));
    L.job->stream = L.st;
    PS_TRY(rt->up(d_pairs, L.dev.data(), L.np * sizeof(SwPair), L.st));
    PS_TRY(rt->up(d_chars, L.job->pool.data(), L.job->pool.size(), L.st));
    PS_HIP(hipMemsetAsync(L.dv.res, 0, L.res_bytes(), L.st));
    PS_HIP(hipMemsetAsync(L.dv.blk, 0, L.tot.blk * sizeof(int), L.st));   // waves beyond a pair's last column never write theirs
    PS_HIP(hipMemsetAsync(d_prog, 0, L.nprog * sizeof(int), L.st));
    return PS_OK;
}

// stage 4: the full-matrix pairs, then the band pairs: one fill and one traceback launch each
static int run(Launch& L) {
    Runtime* rt = L.rt;
    if (rt->prof_on) PS_HIP(hipEventRecord(rt->sw0, L.st));
    bool packed_all = true;   // every pair of the batch on a packed 8-column fill (the band fill is one)
    if (L.nf) {
        // the packed 16-bit fill serves the 8-column build whenever every pair's scores fit 16 bits
        bool packed = L.K == 8 && L.WW == SWW && packed_allowed();
        for (int k = 0; k < L.nf && packed; k++) if (std::min(L.dev[k].n1, L.dev[k].n2) > SW_PK_MAXLEN) packed = false;
        packed_all = packed;
        PS_TRY(sw_run(L.st, L.dv, L.nf, L.nss, L.K, L.WW, packed, false, L.form));
    }
    if (L.nb) {
        SwDev band = L.dv;
        band.pairs += L.nf;
        PS_TRY(sw_run(L.st, band, L.nb, L.nss, 8, SWBW, true, true, L.form));
        if (rt->prof_on) rt->prof["sw_band"].launches++;
    }
    if (rt->prof_on && packed_all) rt->prof["sw_pk8"].launches++;   // (which fill ran: a host-side count per batch, no event pair)
    if (rt->prof_on) rt->prof[L.form == SW_LISTS ? "sw_lists" : (L.form == SW_MAP ? "sw_map" : "sw_summary")].launches++;   // (and which traceback form)
    if (rt->prof_on) PS_HIP(hipEventRecord(rt->sw1, L.st));
    return PS_OK;
}

// stage 5: the records, and in list form the index lists, on their way to pinned host memory
static int queue_copies(Launch& L) {
    Runtime* rt = L.rt;
    PS_TRY(rt->hbuf("sw_res").ensure(L.res_bytes()));
    L.job->res = rt->hbuf("sw_res").as<int>();
    PS_HIP(hipMemcpyAsync(L.job->res, L.dv.res, L.res_bytes(), hipMemcpyDeviceToHost, L.st));
    if (L.form == SW_LISTS) {
        const size_t bytes = (size_t)L.tot.out * sizeof(int);
        PS_TRY(rt->hbuf("sw_out").ensure(bytes));
        L.job->outbuf = rt->hbuf("sw_out").as<int>();
        PS_HIP(hipMemcpyAsync(L.job->outbuf, L.dv.out, bytes, hipMemcpyDeviceToHost, L.st));
    }
    return PS_OK;
}

int sw_launch(Runtime* rt, const SwInput& in, SwJob* job, const int* wbs, SwForm form) {
    Launch L{rt, in, job, form, (int)in.size()};
    if (form == SW_MAP && L.np && !job->d_map) return fail(PS_ERR_BAD_ARG, "Smith-Waterman (map form): no table buffer");
    job->np = L.np;
    job->form = form;
    if (!L.np) return PS_OK;
    for (int k = 0; k < L.np; k++) L.wb.push_back(wbs ? wbs[k] : sw_band_choice(*in[k].first, *in[k].second));
    choose_form(L);
    lay_out(L);
    PS_TRY(place(L));
    PS_TRY(run(L));
    return queue_copies(L);
}

// -------------------------------------------------------------------------------------------------
// sw_finish, in stages.  stage 1: the batch has run, and no strip of it gave up
static int check(Runtime* rt, SwJob* job) {
    PS_HIP(hipStreamSynchronize(job->stream));
    if (rt->prof_on) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, rt->sw0, rt->sw1) == hipSuccess) {
            Prof& pr = rt->prof["sw"];
            pr.ms += ms; pr.launches += 1; pr.bytes += job->cells * 5.0;  // 4-byte score + 1-byte step per cell (the reference's footprint)
        }
    }
    for (const SwPair& p : job->pairs)
        if (sw_rec(sw_record(job->res, p), SWR_TIMED_OUT)) return fail(PS_ERR_HIP, "Smith-Waterman: a strip gave up waiting for its left neighbour (result discarded)");
    return PS_OK;
}

// stage 2: every pair's result in the job's form
static void collect(const SwJob* job, std::vector<SwResult>* out) {
    for (int k = 0; k < job->np; k++) {
        const SwPair& p = job->pairs[k];
        const int* rec = sw_record(job->res, p);
        auto get = [&](SwRec f) { return sw_rec(rec, f); };
        SwResult& r = (*out)[k];
        r.score = get(SWR_SCORE);
        r.n_pairs = get(SWR_N_PAIRS); r.n_match = get(SWR_N_MATCH);
        if (job->form == SW_SUMMARY) {
            r.first1 = get(SWR_FIRST1); r.first2 = get(SWR_FIRST2); r.last1 = get(SWR_LAST1); r.last2 = get(SWR_LAST2);
            r.gap1 = get(SWR_GAP1); r.gap2 = get(SWR_GAP2);
        } else if (job->form == SW_MAP) {
            r.map_lo = get(SWR_MAP_LO); r.map_hi = get(SWR_MAP_HI); r.map_has0 = get(SWR_MAP_HAS0); r.map_y0 = get(SWR_MAP_Y0); r.map_off = p.out_off;
        } else {
            const int* oi = job->outbuf + p.out_off;
            const int* oj = oi + (p.n1 + p.n2 + 2);
            r.a.assign(oi, oi + r.n_pairs); r.b.assign(oj, oj + r.n_pairs);
            std::reverse(r.a.begin(), r.a.end()); std::reverse(r.b.begin(), r.b.end());
        }
        r.accuracy = 100.0 * r.n_match / (double)r.n_pairs;  // NaN for an empty alignment, as the reference computes it
    }
}

// the band pairs whose certificate failed, the band counters and the trace line
static std::vector<int> band_census(const SwJob* job) {
    std::vector<int> failed;
    int edge = 0;
    for (int k = 0; k < job->np; k++) {
        const SwPair& p = job->pairs[k];
        const int* rec = sw_record(job->res, p);
        auto get = [&](SwRec f) { return sw_rec(rec, f); };
        if (!p.wb) continue;
        if (get(SWR_INEXACT)) { failed.push_back(k); continue; }
        if (get(SWR_SCORE) > 0 && std::abs(get(SWR_BI) - get(SWR_BJ)) > p.wb - 64) edge++;
    }
    g_band[0] += job->nband; g_band[1] += (int64_t)failed.size(); g_band[2] += edge;
    g_band[3] += (int64_t)job->band_cells; g_band[4] += (int64_t)job->cells;
    if (trace_on() && job->nband)
        fprintf(stderr, "[ps] smith-waterman band: %d of %d pairs banded, %zu fell back, %d maxima near a band edge, %.3g of %.3g cells\n",
                job->nband, job->np, failed.size(), edge, job->band_cells, job->cells);
    return failed;
}

// stage 3: the pairs whose band certificate failed, on the full matrix, in one follow-up batch in the job's form (the job's staging
// is free again after the sync of stage 1)
static int redo(Runtime* rt, SwJob* job, std::vector<SwResult>* out) {
    const std::vector<int> failed = band_census(job);
    if (failed.empty()) return PS_OK;
    std::vector<std::string> s;
    for (int k : failed) {
        const SwPair& p = job->pairs[k];
        s.emplace_back(job->pool, (size_t)p.s1_off, (size_t)p.n1);
        s.emplace_back(job->pool, (size_t)p.s2_off, (size_t)p.n2);
    }
    SwInput in2;
    for (size_t k = 0; k < failed.size(); k++) in2.push_back({&s[2 * k], &s[2 * k + 1]});
    const std::vector<int> full(failed.size(), 0);
    std::vector<SwResult> part;
    // (map form: the tables go to a buffer of their own and from there to the pairs' places)
    int* d_redo = nullptr;
    if (job->form == SW_MAP) {
        PS_TRY(rt->buf("sw_map_redo").ensure((size_t)sw_map_ints(in2, 0, in2.size()) * sizeof(int)));
        d_redo = rt->buf("sw_map_redo").as<int>();
    }
    PS_TRY(sw_batch(rt, in2, &part, full.data(), job->form, d_redo));
    for (size_t k = 0; k < failed.size(); k++) {
        const SwPair& p = job->pairs[failed[k]];
        if (job->form == SW_MAP) {
            PS_HIP(hipMemcpyAsync(job->d_map + p.out_off, d_redo + part[k].map_off, ((size_t)p.n1 + 2) * sizeof(int), hipMemcpyDeviceToDevice, job->stream));
            part[k].map_off = p.out_off;
        }
        (*out)[failed[k]] = std::move(part[k]);
    }
    if (job->form == SW_MAP) PS_HIP(hipStreamSynchronize(job->stream));
    return PS_OK;
}

int sw_finish(Runtime* rt, SwJob* job, std::vector<SwResult>* out) {
    out->assign(job->np, SwResult());
    if (!job->np) return PS_OK;
    PS_TRY(check(rt, job));
    collect(job, out);
    return redo(rt, job, out);
}

int64_t sw_map_ints(const SwInput& in, size_t k0, size_t k1) {
    int64_t t = 0;
    for (size_t k = k0; k < k1; k++) t += (int64_t)in[k].first->size() + 2;
    return t;
}

int sw_batch(Runtime* rt, const std::vector<std::pair<const std::string*, const std::string*>>& in, std::vector<SwResult>* out, const int* wb, SwForm form, int* d_map) {
    SwJob job;
    job.d_map = d_map;
    PS_TRY(sw_launch(rt, in, &job, wb, form));
    return sw_finish(rt, &job, out);
}

// The checkpoint rows / columns of a batch (~13 MB per full-matrix 10 kb pair) are a pool like the DP matrices: at most PLAN_SW_PART-th of
// this runtime's share goes into one launch.  sw_chunk_end: one past the last pair of the chunk that starts at k0 under `cap` bytes
// (always at least one pair).
size_t sw_chunk_end(const SwInput& in, const int* wbs, SwForm form, size_t k0, double cap) {
    double acc = 0;
    size_t k = k0;
    for (; k < in.size(); k++) {
        const double add = sw_pair_bytes((int)in[k].first->size(), (int)in[k].second->size(), wbs[k], form);
        if (k > k0 && acc + add > cap) break;
        acc += add;
    }
    return k;
}

double sw_chunk_cap() { return device_share_bytes() / PLAN_SW_PART; }

// pairs k0 .. end, chunk after chunk, appended to `out`; a chunk the device has no memory for is cut in two
int sw_chunks(Runtime* rt, const SwInput& in, const int* wbs, SwForm form, size_t k0, std::vector<SwResult>* out, int* nchunks, int* d_map) {
    double cap = sw_chunk_cap();
    while (k0 < in.size()) {
        const size_t k1 = sw_chunk_end(in, wbs, form, k0, cap);
        std::vector<SwResult> part;
        const int64_t map0 = form == SW_MAP ? sw_map_ints(in, 0, k0) : 0;   // the chunk's tables inside d_map
        const int rc = sw_batch(rt, SwInput(in.begin() + k0, in.begin() + k1), &part, wbs + k0, form, d_map ? d_map + map0 : nullptr);
        if (rc == PS_ERR_NOMEM && k1 - k0 > 1) { cap *= 0.5; continue; }
        PS_TRY(rc);
        for (SwResult& r : part) { r.map_off += map0; out->push_back(std::move(r)); }
        if (nchunks) ++*nchunks;
        k0 = k1;
    }
    return PS_OK;
}

int sw_summaries(Runtime* rt, const SwInput& in, std::vector<SwResult>* out) {
    out->clear();
    std::vector<int> wbs(in.size());
    for (size_t k = 0; k < in.size(); k++) wbs[k] = sw_band_choice(*in[k].first, *in[k].second);
    int nchunks = 0;
    PS_TRY(sw_chunks(rt, in, wbs.data(), SW_SUMMARY, 0, out, &nchunks));
    if (trace_on()) fprintf(stderr, "[ps] smith-waterman summaries: %zu pairs in %d chunks\n", in.size(), nchunks);
    return PS_OK;
}

int sw_device(Runtime* rt, const std::string& s1, const std::string& s2, int* score, double* accuracy,
              std::vector<int>* inds1, std::vector<int>* inds2) {
    std::vector<std::pair<const std::string*, const std::string*>> in(1, {&s1, &s2});
    std::vector<SwResult> out;
    PS_TRY(sw_batch(rt, in, &out));
    *score = out[0].score; *accuracy = out[0].accuracy;
    inds1->swap(out[0].a); inds2->swap(out[0].b);
    return PS_OK;
}

}  // namespace ps
