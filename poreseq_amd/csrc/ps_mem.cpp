// ps_mem.cpp — the device-memory plan of libporeseq_hip.so and everything that allocates for it: the runtimes' grow-only pools (DBuf)
// and pinned host memory (HBuf, the staging arena), the count of what the pools of this process hold and its two ceilings, each
// runtime's share, the slabs for full score matrices and the cache of AlignData slabs.  The plan's numbers and formulas are in
// ps_plan.h; every hipMalloc and hipFree of the library is in this file.
#include "ps_host.h"
#include "ps_poison.h"

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>

namespace ps {

static size_t trim_idle_runtimes();   // below: hands back the device pools of runtimes no thread owns
static size_t device_total_bytes();
static size_t device_plan_bytes();   // this process's part of it (ps_set_device_fraction)

// ---- pool accounting: device memory held by the pools of all runtimes and by the slabs -----------------------------------------
// (kept by DBuf::ensure / release and slab_acquire alone; the AlignData slab cache below is not counted)
static std::atomic<long long> g_pool_bytes(0);
static void pool_add(size_t bytes) { g_pool_bytes += (long long)bytes; }
static long long pool_bytes() { return g_pool_bytes.load(); }
// never into the last 6 % of the device: a launch that finds no memory for the HSA runtime's own needs aborts the process
// (HSA_STATUS_ERROR_OUT_OF_RESOURCES) — DBuf::ensure refuses instead, callers that can cut their batch do so on PS_ERR_NOMEM
static bool pools_over_ceiling(size_t want, size_t tot) { return (double)g_pool_bytes.load() + (double)want > PLAN_POOL_CEILING * (double)tot; }
// the matrix pools `rec` and `flg` re-sized to need_rec and need_flg bytes would reach into the last 8 % (ensure_matrix_pools)
static bool matrices_over_ceiling(const DBuf& rec, const DBuf& flg, size_t need_rec, size_t need_flg, size_t tot) {
    return (double)(g_pool_bytes.load() - (long long)rec.cap - (long long)flg.cap) + (double)need_rec + (double)need_flg > PLAN_MATRIX_CEILING * (double)tot;
}

hipError_t DBuf::release() {
    if (!p) return hipSuccess;
    const hipError_t e = hipFree(p);   // (a failure leaves nothing to retry with: pointer and count go either way)
    g_pool_bytes -= (long long)cap;
    p = nullptr; cap = 0;
    return e;
}

int DBuf::ensure(size_t bytes) {
    if (bytes <= cap && p) return PS_OK;
    if (trace_on()) fprintf(stderr, "[ps] pool grow %zu -> %zu bytes\n", cap, bytes);
    PS_HIP(release());
    size_t want = std::max<size_t>(bytes + std::min<size_t>(bytes / 4, (size_t)1 << 30), 1 << 16);   // growth slack, at most 1 GB
    if (const size_t tot = device_plan_bytes()) {
        auto over = [&](size_t w) { return pools_over_ceiling(w, tot); };
        if (over(want)) want = std::max<size_t>(bytes, 1 << 16);
        if (over(want)) (void)trim_idle_runtimes();
        if (over(want))
            return fail(PS_ERR_NOMEM, "device pools of this process would reach " + std::to_string((size_t)((pool_bytes() + (long long)want) >> 20)) + " MB of " +
                                      std::to_string(tot >> 20) + " MB (a buffer of " + std::to_string(want >> 20) + " MB was asked for)");
    }
    if (hipMalloc(&p, want) != hipSuccess) {
        p = nullptr;
        (void)hipGetLastError();   // (sticky: the next launch check would report it)
        want = std::max<size_t>(bytes, 1 << 16);
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) {
            // runtimes on the free list (their threads are gone) keep their pools for the next thread: take them back first
            (void)hipGetLastError();
            const size_t got = trim_idle_runtimes();
            if (trace_on()) fprintf(stderr, "[ps] out of device memory: %zu bytes taken back from idle runtimes\n", got);
            p = nullptr;
            e = got ? hipMalloc(&p, want) : e;
        }
        if (e != hipSuccess) { p = nullptr; (void)hipGetLastError(); 
            size_t fr = 0, tt = 0;
            (void)hipMemGetInfo(&fr, &tt);
            return fail(PS_ERR_NOMEM, std::string("hipMalloc of ") + std::to_string(want >> 20) + " MB: " + hipGetErrorString(e) + " (" + std::to_string(fr >> 20) + " of " +
                                      std::to_string(tt >> 20) + " MB free, " + std::to_string((long long)(pool_bytes() >> 20)) + " MB in this process's pools)");
        }
    }
    cap = want;
    pool_add(cap);
    return PS_OK;
}

int HBuf::ensure(size_t bytes) {
    if (bytes <= cap && p) return PS_OK;
    if (p) { PS_HIP(hipHostFree(p)); p = nullptr; cap = 0; }
    const size_t want = std::max<size_t>(bytes + bytes / 4, 1 << 16);
    PS_HIP(hipHostMalloc(&p, want, hipHostMallocDefault));
    cap = want;
    return PS_OK;
}

void* Stage::alloc(size_t bytes) {
    bytes = (std::max<size_t>(bytes, 1) + 255) & ~(size_t)255;
    if (chunks.empty() || used + bytes > chunks.back().cap) {
        size_t want = std::max<size_t>(bytes, chunks.empty() ? (size_t)4 << 20 : 2 * chunks.back().cap);
        void* p = nullptr;
        if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) {
            want = bytes;
            if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) return nullptr;
        }
        chunks.push_back({(char*)p, want});
        used = 0;
    }
    void* r = chunks.back().p + used;
    used += bytes;
    dirty = true;
    return r;
}

int Stage::reset() {
    if (chunks.size() > 1) {   // grew during the last call: one chunk of the combined size from now on
        size_t tot = 0;
        for (Chunk& c : chunks) { tot += c.cap; PS_HIP(hipHostFree(c.p)); }
        chunks.clear();
        void* p = nullptr;
        if (hipHostMalloc(&p, tot, hipHostMallocDefault) == hipSuccess) chunks.push_back({(char*)p, tot});
    }
    used = 0;
    dirty = false;
    return PS_OK;
}

int Runtime::up(void* dst, const void* src, size_t bytes, hipStream_t st) {
    if (!bytes) return PS_OK;
    void* h = stage.alloc(bytes);
    if (!h) return fail(PS_ERR_NOMEM, "hipHostMalloc (staging arena)");
    memcpy(h, src, bytes);
    PS_HIP(hipMemcpyAsync(dst, h, bytes, hipMemcpyHostToDevice, st ? st : stream));
    return PS_OK;
}

int Runtime::down(void** hptr, const void* src, size_t bytes, hipStream_t st) {
    void* h = stage.alloc(bytes);
    if (!h) return fail(PS_ERR_NOMEM, "hipHostMalloc (staging arena)");
    *hptr = h;
    if (bytes) PS_HIP(hipMemcpyAsync(h, src, bytes, hipMemcpyDeviceToHost, st ? st : stream));
    return PS_OK;
}

static size_t trim_idle_runtimes() {
    size_t got = 0;
    for_idle_runtimes([&](Runtime& R) {
        for (auto& kv : R.pool) {
            const size_t cap = kv.second.cap;
            if (kv.second.release() == hipSuccess) got += cap;   // (the owning thread drained its streams before it left)
        }
    });
    return got;
}

// ---- what this process plans for ----------------------------------------------------------------------------------------------
static size_t device_total_bytes() {
    static std::atomic<size_t> dev_total(0);       // the device's memory size does not change: asked once
    size_t tot = dev_total.load();
    if (!tot) {
        size_t fr = 0;
        if (hipMemGetInfo(&fr, &tot) != hipSuccess || !tot) return 0;
        dev_total.store(tot);
    }
    return tot;
}

// The part of the device this PROCESS plans for.  One process per GPU (the normal deployment) owns the device: 1.  Several ranks on one
// device (poreseq_amd.dist.init with more ranks than GPUs; the 8-rank test of the driver's command line on one GPU) each plan for
// their fraction — ps_set_device_fraction / PORESEQ_DEVICE_FRACTION — so that the slabs, the runtimes' shares and the 94 % guard of
// the pools add up to one device, not to one device per rank.
static std::atomic<double> g_dev_fraction(-1.0);
void device_fraction_set(double f) { g_dev_fraction.store(f > 0.0 && f <= 1.0 ? f : -1.0); }
double device_fraction() {
    const double f = g_dev_fraction.load();
    if (f > 0.0) return f;
    static const double env = [] { const char* e = getenv("PORESEQ_DEVICE_FRACTION"); const double v = e ? atof(e) : 1.0; return v > 0.0 && v <= 1.0 ? v : 1.0; }();
    return env;
}
static size_t device_plan_bytes() { return (size_t)(device_fraction() * (double)device_total_bytes()); }

// This runtime's share of the device memory (ps_plan.h): PORESEQ_MAX_BATCH_GB when set, otherwise the plan's formula over the most
// threads that owned a runtime at once (forgotten a minute after the count was last that high).  Within a run of a multi-threaded
// driver the count only goes up, so shares only go down: pools sized under a larger share are given back at the owner's next
// Batch::place, and after the first step every pool fits its share (no regrowth, no thrash).
// PORESEQ_MAX_BATCH_GB in bytes (read at every call: tests change it); 0: set without a budget, < 0: not set
static double max_batch_env() { const char* e = getenv("PORESEQ_MAX_BATCH_GB"); return e ? std::max(atof(e), 0.0) * 1e9 : -1.0; }
double device_share_bytes() {
    if (const double g = max_batch_env(); g > 0) return g;
    const size_t tot = device_plan_bytes();
    if (!tot) return 32e9;
    return share_bytes(tot, peak_runtimes());
}

// ---- slabs for full score matrices -----------------------------------------------------------------------------------------
// Only a ScoreMutations call whose edit list reads most columns (Refine / ScorePoints: point edits at every position, ~4 % of a
// consensus schedule's calls) keeps full forward + backward matrices: 265 MB per 10 kb event, 53 GB for a lock-step call of 20
// regions.  Sizing every runtime's pools for that (round 3: 65 % of the device divided by the batches in flight) made the number of
// batches in flight a memory question.  Instead the process keeps a few slabs (PORESEQ_SLABS, default PLAN_SLABS, of PORESEQ_SLAB_GB,
// default 9 % of the device each: 28 GB on an MI355X = the matrices of 10 regions per launch), allocated on first use and never
// freed; a dense call takes one for its
// duration (fills, backtrace, edit scoring, read-back) and waits when all are taken.  Nothing is acquired while a slab is held.
// A single AlignData whose matrices exceed a slab (a 48 kb region with 30 events: 41 GB) takes the calling runtime's own pools.
namespace {
struct Slab { char* p = nullptr; size_t bytes = 0; bool busy = false; };
std::mutex g_slab_mu;
std::condition_variable g_slab_cv;
std::vector<Slab*> g_slabs;
}  // namespace
static int slab_count() { static const int n = getenv("PORESEQ_SLABS") ? std::max(1, atoi(getenv("PORESEQ_SLABS"))) : PLAN_SLABS; return n; }
size_t slab_bytes() {
    static const double gb = getenv("PORESEQ_SLAB_GB") ? atof(getenv("PORESEQ_SLAB_GB")) : 0.0;
    if (gb > 0) return (size_t)(gb * 1e9);
    const size_t tot = device_plan_bytes();
    return tot ? slab_default_bytes(tot) : (size_t)24e9;
}
// bytes of full matrices one dense call may place: the slab, or PORESEQ_MAX_BATCH_GB when set (tests: tiny budgets)
double dense_cap_bytes() {
    // (the smallest slab actually allocated, when one came out smaller than planned: sub-batches are cut to fit any of them)
    size_t cap = slab_bytes();
    { std::lock_guard<std::mutex> lk(g_slab_mu); for (const Slab* sl : g_slabs) cap = std::min(cap, sl->bytes); }
    if (const double g = max_batch_env(); g > 0) return std::min(g, (double)cap);
    return (double)cap;
}
void SlabHold::release() {
    if (!s) return;
    if (drain) (void)hipStreamSynchronize(drain);   // (a no-op on the normal path: the call has read its results back)
    { std::lock_guard<std::mutex> lk(g_slab_mu); ((Slab*)s)->busy = false; }
    s = nullptr; p = nullptr; bytes = 0;
    g_slab_cv.notify_one();
}
int slab_acquire(SlabHold* h) {
    std::unique_lock<std::mutex> lk(g_slab_mu);
    for (;;) {
        for (Slab* sl : g_slabs) if (!sl->busy) { sl->busy = true; h->s = sl; h->p = sl->p; h->bytes = sl->bytes; return PS_OK; }
        if ((int)g_slabs.size() < slab_count()) {
            Slab* sl = new Slab();
            size_t want = slab_bytes();
            hipError_t e = hipMalloc((void**)&sl->p, want);
            if (e != hipSuccess) {   // the device is fuller than expected: idle runtimes' pools first, then a smaller slab
                (void)hipGetLastError();
                (void)trim_idle_runtimes();
                for (int k = 0; k < 3 && e != hipSuccess; k++) { if (k) want = want / 4 * 3; e = hipMalloc((void**)&sl->p, want); if (e != hipSuccess) (void)hipGetLastError(); }
            }
            if (e != hipSuccess) {
                delete sl;
                if (!g_slabs.empty()) { g_slab_cv.wait(lk); continue; }   // make do with the slabs there are
                return fail(PS_ERR_NOMEM, std::string("hipMalloc of a ") + std::to_string(want >> 20) + " MB slab for full score matrices: " + hipGetErrorString(e));
            }
            sl->bytes = want; sl->busy = true;
            pool_add(want);
            g_slabs.push_back(sl);
            h->s = sl; h->p = sl->p; h->bytes = sl->bytes;
            return PS_OK;
        }
        g_slab_cv.wait(lk);
    }
}

// The DP matrices ("rec": 16-byte records, or a strip sweep's step codes, which alias it; "flg": step words) are the only big pools,
// and several runtimes size theirs at different times (the share depends on how many threads are inside the library).  Two rules
// keep the sum below the device: a runtime whose pools were sized for a much larger share than today's gives them back before
// re-sizing, and no matrix pool grows into the last 8 % of the device (small buffers of every runtime live there) — PS_ERR_NOMEM
// instead, which callers that can split turn into smaller batches.
int ensure_matrix_pools(Runtime* rt, const Batch& bt, size_t need_rec, size_t need_flg, bool can_split, void** rec_out, void** flg_out) {
    if (bt.ext) {   // full matrices of a dense ScoreMutations call: carved out of the slab the caller holds
        const size_t r = (need_rec + 255) & ~(size_t)255;
        if (r + need_flg > bt.ext_bytes)
            return fail(PS_ERR_NOMEM, "the score matrices of this call (" + std::to_string((r + need_flg) >> 20) + " MB) do not fit a slab of " + std::to_string(bt.ext_bytes >> 20) +
                                      " MB (PORESEQ_SLAB_GB)");
        *rec_out = bt.ext; *flg_out = bt.ext + r;
        return PS_OK;
    }
    DBuf& rec = rt->buf("rec");
    DBuf& flg = rt->buf("flg");
    size_t tot = device_plan_bytes();
    if (max_batch_env() < 0 && rec.p && (double)rec.cap > 1.5 * device_share_bytes() + 2e9 && need_rec < rec.cap) {
        PS_HIP(hipStreamSynchronize(rt->stream));
        PS_HIP(rec.release());
        PS_HIP(flg.release());
    }
    if (tot && (need_rec > rec.cap || need_flg > flg.cap)) {
        auto over = [&] { return matrices_over_ceiling(rec, flg, need_rec, need_flg, tot); };
        if (over()) (void)trim_idle_runtimes();
        if (over() && can_split) return fail(PS_ERR_NOMEM, "the DP matrices of this batch do not fit beside the pools of the other threads' batches");
    }
    PS_TRY(rec.ensure(need_rec));
    if (need_flg) PS_TRY(flg.ensure(need_flg));
    *rec_out = rec.p; *flg_out = flg.p;
    return PS_OK;
}

// ---- AlignData slab cache --------------------------------------------------------------------------------------------------
// The slab of an AlignData (events, derived tables, results: ~13 MB for a 10 kb region at 10x) comes from a process-wide cache and goes
// back to it.  hipFree waits for EVERY stream of the process (43 ms per call with fourteen lock-step batches in flight: 280 regions per
// bench step were 12 s of blocked slot threads), hipMalloc takes ~2 ms; a cached slab costs an event: recorded on the stream that
// last had work on the slab when its AlignData goes, waited for (on the device, not the host) by the stream of the next owner.
namespace {
struct CachedSlab { void* p; size_t cap; hipEvent_t ev; bool pending; };
std::mutex g_aslab_mu;
std::vector<CachedSlab> g_aslabs;
size_t g_aslab_bytes = 0;
size_t aslab_cache_limit() {
    // PLAN_ALIGN_CACHE_MAX, at most PLAN_ALIGN_CACHE_FRAC of this process's part of the device (ranks that share a GPU: ps_set_device_fraction)
    static const double env = getenv("PORESEQ_ALIGN_CACHE_GB") ? atof(getenv("PORESEQ_ALIGN_CACHE_GB")) * 1e9 : -1.0;
    if (env >= 0) return (size_t)env;
    const size_t plan = device_plan_bytes();
    return plan ? align_cache_default(plan) : (size_t)PLAN_ALIGN_CACHE_MAX;
}
}  // namespace

// the slab of an AlignData that goes: into the cache behind an event on `last_stream` (the stream that last had work on it), or freed
void align_slab_give(void* slab, size_t slab_cap, void* last_stream) {
    if (!slab) return;
    CachedSlab c{slab, slab_cap, nullptr, false};
    bool keep = slab_cap > 0 && hipEventCreateWithFlags(&c.ev, hipEventDisableTiming) == hipSuccess;
    if (keep && last_stream) {
        if (hipEventRecord(c.ev, (hipStream_t)last_stream) == hipSuccess) c.pending = true;
        else { (void)hipGetLastError(); (void)hipEventDestroy(c.ev); keep = false; }
    }
    if (keep) {
        std::lock_guard<std::mutex> lk(g_aslab_mu);
        if (g_aslab_bytes + c.cap <= aslab_cache_limit()) { g_aslabs.push_back(c); g_aslab_bytes += c.cap; return; }
    }
    if (keep) (void)hipEventDestroy(c.ev);
    (void)hipFree(slab);
}

// a slab of at least `bytes` for an AlignData on `rt`'s stream: the smallest cached one that fits without wasting more than half of
// itself, else a fresh allocation (with an eighth of slack, so that regions of similar size find each other's slabs)
int align_slab_take(Runtime* rt, size_t bytes, void** out, size_t* cap) {
    CachedSlab got{nullptr, 0, nullptr, false};
    {
        std::lock_guard<std::mutex> lk(g_aslab_mu);
        int best = -1;
        for (int k = 0; k < (int)g_aslabs.size(); k++)
            if (g_aslabs[k].cap >= bytes && g_aslabs[k].cap <= 2 * bytes + (1 << 20) && (best < 0 || g_aslabs[k].cap < g_aslabs[best].cap)) best = k;
        if (best >= 0) { got = g_aslabs[best]; g_aslabs[best] = g_aslabs.back(); g_aslabs.pop_back(); g_aslab_bytes -= got.cap; }
    }
    if (got.p) {
        if (got.pending) PS_HIP(hipStreamWaitEvent(rt->stream, got.ev, 0));   // (the previous owner's last work on it, if any is still queued)
        (void)hipEventDestroy(got.ev);   // (destruction is deferred by the runtime until the wait above has been honoured)
        *out = got.p; *cap = got.cap;
        return PS_OK;
    }
    const size_t want = (bytes + bytes / 8 + ((size_t)1 << 20) - 1) >> 20 << 20;
    if (hipMalloc(out, want) != hipSuccess) {
        (void)hipGetLastError();
        {   // hand the cache back and try once more
            std::lock_guard<std::mutex> lk(g_aslab_mu);
            for (CachedSlab& c : g_aslabs) { (void)hipEventDestroy(c.ev); (void)hipFree(c.p); }
            g_aslabs.clear(); g_aslab_bytes = 0;
        }
        PS_HIP(hipMalloc(out, want));
    }
    *cap = want;
    return PS_OK;
}
// ---- ps_debug_poison: overwrite what the calling thread's next call could find left over -----------------------------------------
// A test hook (ps_poison.h has the class of every pool).  Plain vector stores; tails that are no multiple of 16 bytes word by word.
__global__ void k_poison(uint4* __restrict__ p, size_t n16, size_t tail_words, size_t tail_bytes, unsigned lo, unsigned hi) {
    const size_t step = (size_t)gridDim.x * blockDim.x;
    const size_t t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (size_t i = t0; i < n16; i += step) p[i] = make_uint4(lo, hi, lo, hi);
    unsigned* w = (unsigned*)(p + n16);
    if (t0 < tail_words) w[t0] = (t0 & 1) ? hi : lo;
    unsigned char* c = (unsigned char*)(w + tail_words);
    if (t0 < tail_bytes) c[t0] = (unsigned char)lo;
}
static int poison_device(Runtime* rt, void* p, size_t bytes, unsigned lo, unsigned hi) {
    if (!p || !bytes) return PS_OK;
    const size_t n16 = bytes / 16, rest = bytes % 16;
    const unsigned blocks = (unsigned)std::min<size_t>(std::max<size_t>((n16 + 255) / 256, 1), 256 * 64);
    hipLaunchKernelGGL(k_poison, dim3(blocks), dim3(256), 0, rt->stream, (uint4*)p, n16, rest / 4, rest % 4, lo, hi);
    PS_LAUNCH_CHECK();
    return PS_OK;
}
static void poison_host(void* p, size_t bytes, unsigned word) {
    if (!p) return;
    unsigned* w = (unsigned*)p;
    std::fill(w, w + bytes / 4, word);
    memset((char*)p + bytes / 4 * 4, (int)(word & 255), bytes % 4);
}

int debug_poison(Runtime* rt, uint32_t index_word, uint64_t value_word, ps_poison_report* rep, int32_t cap, int32_t* n_rep) {
    int n = 0;
    auto say = [&](const std::string& name, size_t bytes, PoisonClass cls, int skipped) {
        if (rep && n < cap) {
            ps_poison_report& r = rep[n];
            memset(&r, 0, sizeof(r));
            strncpy(r.name, name.c_str(), sizeof(r.name) - 1);
            r.bytes = (int64_t)bytes; r.cls = (int32_t)cls; r.skipped = skipped;
        }
        n++;
    };
    // nothing of this thread's may be in flight, and nothing it staged may still be wanted
    PS_HIP(hipStreamSynchronize(rt->stream));
    if (rt->stream2) PS_HIP(hipStreamSynchronize(rt->stream2));
    const unsigned vlo = (unsigned)(value_word & 0xffffffffu), vhi = (unsigned)(value_word >> 32);
    for (auto& kv : rt->pool) {
        const PoisonEntry* e = poison_entry(kv.first.c_str());
        const PoisonClass cls = e ? e->cls : PoisonClass::INDEX;
        if (cls == PoisonClass::EXEMPT) { say(kv.first, 0, cls, kv.second.p ? 1 : 0); continue; }
        const bool val = cls == PoisonClass::VALUE;
        PS_TRY(poison_device(rt, kv.second.p, kv.second.cap, val ? vlo : index_word, val ? vhi : index_word));
        say(kv.first, kv.second.p ? kv.second.cap : 0, cls, 0);
    }
    {   // the dense slabs no call holds (the lock is kept over the fill: a taker must not start before it has run)
        std::lock_guard<std::mutex> lk(g_slab_mu);
        size_t bytes = 0;
        int busy = 0;
        for (Slab* sl : g_slabs) {
            if (sl->busy) { busy++; continue; }
            PS_TRY(poison_device(rt, sl->p, sl->bytes, index_word, index_word));
            bytes += sl->bytes;
        }
        PS_HIP(hipStreamSynchronize(rt->stream));
        say("slab", bytes, PoisonClass::INDEX, busy);
    }
    {   // the cached AlignData slabs, each after the last work of its previous owner (a live AlignData's slab is not in the cache)
        std::lock_guard<std::mutex> lk(g_aslab_mu);
        size_t bytes = 0;
        for (CachedSlab& c : g_aslabs) {
            if (c.pending) PS_HIP(hipEventSynchronize(c.ev));
            PS_TRY(poison_device(rt, c.p, c.cap, index_word, index_word));
            bytes += c.cap;
        }
        PS_HIP(hipStreamSynchronize(rt->stream));
        say("align_cache", bytes, PoisonClass::INDEX, 0);
    }
    for (auto& kv : rt->hpool) {
        poison_host(kv.second.p, kv.second.cap, index_word);
        say("host:" + kv.first, kv.second.p ? kv.second.cap : 0, PoisonClass::INDEX, 0);
    }
    {
        size_t bytes = 0;
        for (Stage::Chunk& c : rt->stage.chunks) { poison_host(c.p, c.cap, index_word); bytes += c.cap; }
        say("stage", bytes, PoisonClass::INDEX, 0);
    }
    if (n_rep) *n_rep = n;
    return PS_OK;
}

// what ps_info's line says about this file's state
MemInfo mem_info() {
    MemInfo m;
    { std::lock_guard<std::mutex> lk(g_slab_mu); m.slabs = g_slabs.size(); for (const Slab* sl : g_slabs) m.slab_bytes += sl->bytes; }
    m.slabs_planned = slab_count();
    m.pool_bytes = pool_bytes();
    return m;
}

}  // namespace ps
