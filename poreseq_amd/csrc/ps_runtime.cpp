// ps_runtime.cpp — process-wide plumbing of libporeseq_hip.so: the last error and the trace timers, the runtime of each host thread
// (HIP streams, events; the free list that hands runtimes from thread to thread), how streams get hardware queues, the kernel
// profile's event pairs, the pool of host threads behind par_for, and ps_info's line.  What a runtime's device pools may hold is
// ps_mem.cpp's business.
#include "ps_host.h"

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <deque>
#include <memory>
#include <mutex>
#include <thread>

namespace ps {

static thread_local std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }
const char* last_error() { return g_err.c_str(); }

static double now_s() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec + 1e-9 * ts.tv_nsec; }
bool trace_on() { static const bool on = getenv("PORESEQ_TRACE") != nullptr; return on; }
Tick::Tick(const char* w) : what(w), t0(now_s()), on(trace_on()) {}
void Tick::lap(const char* label) {
    if (!on) return;
    const double t = now_s();
    fprintf(stderr, "[ps] %-18s %-22s %8.3f ms\n", what, label, 1e3 * (t - t0));
    t0 = t;
}

// One runtime (HIP streams + grow-only device pools) per host thread that is inside the library: independent
// PSAlign pipelines driven from different threads run concurrently on the GPU — a single region keeps at most a
// few dozen of the 256 CUs busy, and regions are independent work-items.  Runtimes live in a process-wide
// free-list: a thread adopts one on its first call and hands it back when it exits, so short-lived worker
// threads reuse the pools instead of re-allocating (or leaking) them.
namespace {
struct RtSlot { Runtime R; int state = 0; std::string why; };   // state: 0 untried, 1 ok, -1 failed
std::mutex g_rt_mu;
std::vector<RtSlot*> g_rt_free;
struct RtHolder {
    RtSlot* s = nullptr;
    ~RtHolder();
};
thread_local RtHolder t_rt;
std::atomic<int> g_rt_live(0);
std::atomic<int> g_rt_peak(0);   // most threads that owned a runtime at the same time (forgotten a minute after the count was last that high)
std::atomic<double> g_rt_peak_at(0.0);
}  // namespace
int live_runtimes() { return g_rt_live.load(); }
int peak_runtimes() {
    // a burst of threads long ago must not shrink a later lone caller's share for good
    const double t = now_s();
    if (t - g_rt_peak_at.load() > 60.0) { g_rt_peak.store(std::max(g_rt_live.load(), 1)); g_rt_peak_at.store(t); }
    return g_rt_peak.load();
}
// the runtimes no thread owns, one after the other, under the free list's lock (trim_idle_runtimes, ps_mem.cpp)
void for_idle_runtimes(const std::function<void(Runtime&)>& fn) {
    std::lock_guard<std::mutex> lk(g_rt_mu);
    for (RtSlot* s : g_rt_free) fn(s->R);
}
RtHolder::~RtHolder() {
    if (!s) return;
    if (getenv("PORESEQ_TRACE")) {   // what this thread's runtime holds, largest first
        std::vector<std::pair<size_t, std::string>> v;
        size_t tot = 0;
        for (auto& kv : s->R.pool) { v.push_back({kv.second.cap, kv.first}); tot += kv.second.cap; }
        std::sort(v.rbegin(), v.rend());
        std::string line = "[ps] runtime handed back: " + std::to_string(tot >> 20) + " MB of device pools:";
        for (size_t k = 0; k < v.size() && k < 12; k++) line += " " + v[k].second + " " + std::to_string(v[k].first >> 20);
        fprintf(stderr, "%s\n", line.c_str());
    }
    std::lock_guard<std::mutex> lk(g_rt_mu);
    g_rt_free.push_back(s);
    g_rt_live--;
}

// How the runtimes' streams get hardware queues (see make_stream below).  GPU_MAX_HW_QUEUES only counts when HIP read it, i.e. when
// it was in the environment before the HIP runtime started: either the process was started with it (/proc/self/environ is the
// environment at exec, later setenv calls do not show there), or the poreseq_amd package exported it at import after checking that
// nothing in the process had opened the GPU yet (it then sets PORESEQ_HWQ_SET_BY_PACKAGE=1).  A value that appeared any other way
// is not trusted: seven streams on four queues of ONE priority level would be the slowest arrangement of all (108 against 141 kb/s).
static int hwq_from_exec_env() {
    static const int v = [] {
        FILE* f = fopen("/proc/self/environ", "rb");
        if (!f) return 0;
        std::string all;
        char buf[4096];
        size_t n;
        while ((n = fread(buf, 1, sizeof buf, f)) > 0) all.append(buf, n);
        fclose(f);
        const std::string key = "GPU_MAX_HW_QUEUES=";
        for (size_t at = 0; at < all.size();) {
            const size_t end = all.find('\0', at);
            const std::string kv = all.substr(at, end == std::string::npos ? std::string::npos : end - at);
            if (kv.compare(0, key.size(), key) == 0) return atoi(kv.c_str() + key.size());
            if (end == std::string::npos) break;
            at = end + 1;
        }
        return 0;
    }();
    return v;
}
// Private queues.  Where HIP runs on its default of four pooled queues per level, a runtime's stream is created with a CU mask of
// the whole device instead: the HIP runtime gives a stream with a CU mask a hardware queue of its own, outside the pool that
// GPU_MAX_HW_QUEUES limits, on the normal priority level.  The process holds at most PORESEQ_PRIVATE_QUEUES of them (default and
// ceiling 16, what the package asks HIP for; 0 switches them off), times the device fraction when several ranks share a GPU.
// A runtime keeps its stream for the life of the process (free list above), so the count follows the most runtimes alive at once.
namespace {
std::atomic<int> g_pq_held(0);   // runtimes whose stream holds a private queue
std::atomic<int> g_pq_fell(0);   // runtimes that were dealt a priority level instead (budget spent, or the create failed)
}  // namespace
static int private_queue_knob() {
    static const int v = [] { const char* e = getenv("PORESEQ_PRIVATE_QUEUES"); return e ? std::max(0, std::min(atoi(e), 16)) : 16; }();
    return v;
}
static int private_queue_budget() {
    const int k = private_queue_knob();
    return k > 0 ? std::max(1, (int)(k * device_fraction() + 1e-9)) : 0;
}
// a stream on a queue of its own when the budget has one left (false: the caller deals a priority level)
static bool private_stream(hipStream_t* st, int cus) {
    const int budget = private_queue_budget();
    int held = g_pq_held.load();
    bool mine = false;
    while (cus > 0 && held < budget && !(mine = g_pq_held.compare_exchange_weak(held, held + 1))) {}
    if (mine) {
        std::vector<uint32_t> mask((size_t)(cus + 31) / 32, 0xffffffffu);   // (ROC_GLOBAL_CU_MASK still applies: HIP intersects the two)
        if (cus % 32) mask.back() = (1u << (cus % 32)) - 1u;
        if (hipExtStreamCreateWithCUMask(st, (uint32_t)mask.size(), mask.data()) == hipSuccess) return true;
        (void)hipGetLastError();
        *st = nullptr;
        g_pq_held--;
    }
    g_pq_fell++;
    return false;
}

int hwq_mode(std::string* why) {
    static int mode = -1;
    static std::string reason;
    static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    if (mode < 0) {
        const char* e = getenv("GPU_MAX_HW_QUEUES");
        const int now = e ? atoi(e) : 0;
        const char* pk = getenv("PORESEQ_HWQ_SET_BY_PACKAGE");
        if (getenv("PORESEQ_ONE_PRIORITY")) { mode = 1; reason = "one priority level (PORESEQ_ONE_PRIORITY)"; }
        else if (getenv("PORESEQ_PRIORITY_LEVELS")) { mode = 0; reason = "streams dealt over the priority levels (PORESEQ_PRIORITY_LEVELS)"; }
        else if (hwq_from_exec_env() >= 8) { mode = 1; reason = "one priority level, a hardware queue per stream (GPU_MAX_HW_QUEUES=" + std::to_string(hwq_from_exec_env()) + " in the process's start-up environment)"; }
        else if (now >= 8 && pk && atoi(pk) == 1) { mode = 1; reason = "one priority level, a hardware queue per stream (GPU_MAX_HW_QUEUES=" + std::to_string(now) + " exported by the poreseq_amd package before HIP started)"; }
        else if (now >= 8) { mode = 0; reason = "streams dealt over the priority levels (GPU_MAX_HW_QUEUES=" + std::to_string(now) + " appeared after start-up without the package's guarantee that HIP had not started: not trusted)"; }
        else if (private_queue_knob() > 0) { mode = 2; reason = "a private hardware queue per stream (CU-masked streams beside HIP's default of 4 hardware queues per level)"; }
        else { mode = 0; reason = "streams dealt over the priority levels (HIP's default of 4 hardware queues per level; private queues switched off by PORESEQ_PRIVATE_QUEUES=0)"; }
    }
    if (why) *why = reason;
    return mode;
}

int second_stream(Runtime* rt, hipStream_t* out) {
    // One stream per runtime as soon as several host threads drive the GPU (lock-step batches in flight): HIP maps streams onto
    // 4 hardware queues by default, and the 5th stream serialises behind another one — measured: 4 batches x 1 stream 101 kb/s,
    // 4 batches x 2 streams 69 kb/s; the overlap a second stream buys comes from the other batches anyway.
    // (PORESEQ_ONE_STREAM forces it for a lone thread too; read once: getenv races with setenv from other threads.)
    static const bool one = getenv("PORESEQ_ONE_STREAM") != nullptr;
    // PORESEQ_FORCE_STREAM2 (diagnostics only, tests/test_hip_variant.py and DESIGN.md section 9): second streams even with
    // several threads inside the library; "prio" puts them on the next stream priority level, as round 2's experiment did
    static const char* force = getenv("PORESEQ_FORCE_STREAM2");
    if (!force && (one || live_runtimes() > 1)) { *out = rt->stream; return PS_OK; }
    if (!rt->stream2 && force && !strcmp(force, "prio")) {
        static std::atomic<int> seq(1);
        int lo = 0, hi = 0;
        if (hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && lo > hi)
            PS_HIP(hipStreamCreateWithPriority(&rt->stream2, hipStreamNonBlocking, hi + seq++ % (lo - hi + 1)));
    }
    if (!rt->stream2) PS_HIP(hipStreamCreateWithFlags(&rt->stream2, hipStreamNonBlocking));
    *out = rt->stream2;
    return PS_OK;
}

int runtime(Runtime** out) {
    if (!t_rt.s) {
        std::lock_guard<std::mutex> lk(g_rt_mu);
        if (!g_rt_free.empty()) { t_rt.s = g_rt_free.back(); g_rt_free.pop_back(); }
        else t_rt.s = new RtSlot();
        {
            const int n = ++g_rt_live;
            int pk = g_rt_peak.load();
            while (n > pk && !g_rt_peak.compare_exchange_weak(pk, n)) {}
            if (n >= g_rt_peak.load()) g_rt_peak_at.store(now_s());
        }
        if (t_rt.s->state == 1) (void)hipSetDevice(t_rt.s->R.device);   // the current device is per-thread state
    }
    Runtime& R = t_rt.s->R;
    int& state = t_rt.s->state;
    std::string& why = t_rt.s->why;
    if (state == 0) {
        int n = 0;
        hipError_t e = hipGetDeviceCount(&n);
        if (e != hipSuccess || n <= 0) {
            state = -1;
            why = std::string("no HIP device available (") + (e != hipSuccess ? hipGetErrorString(e) : "count 0") +
                  "); libporeseq_hip has no CPU fallback";
        } else {
            int dev = 0;
            if (const char* s = getenv("PORESEQ_DEVICE")) dev = atoi(s);
            else if (const char* s2 = getenv("LOCAL_RANK")) dev = atoi(s2) % n;
            if (dev < 0 || dev >= n) dev = 0;
            hipDeviceProp_t prop;
            // One non-blocking stream for the alignment pipeline; a second one for Smith-Waterman batches (they
            // overlap with the base realign inside FindMutations) is created on first use (second_stream()).
            // Partitioning the CUs between them (hipExtStreamCreateWithCUMask) was measured and made no
            // difference, so it is not used.
            // Streams and hardware queues.  HIP multiplexes a process's streams onto GPU_MAX_HW_QUEUES hardware queues per stream
            // priority level (default 4), and streams that share a queue run their kernels one after the other: seven lock-step
            // batches on one level = seven streams on four queues, three kernels in flight on average, 108 kb/s.
            //  * GPU_MAX_HW_QUEUES >= 8 in force (hwq_mode() above: in the environment the process started with, or exported by the
            //    poreseq_amd package before HIP started): every runtime's stream on the default level, a queue each — 146-147 kb/s.
            //  * a value that is not trusted, no private queue to be had (below), or PORESEQ_PRIORITY_LEVELS: the streams are dealt
            //    round-robin to the device's three priority levels, not for the priorities' sake but
            //    for the 3 x 4 queues: 141 kb/s — the two or three batches on the lowest level finish ~0.8 s after the others
            //    (profiles/r03_d_sweep_forms.md).
            //  * HIP on its default (no value, or one below 8): a private queue per runtime while the budget lasts (private_stream()
            //    above: a stream with a CU mask of the whole device; it is blocking with respect to the null stream, which the library
            //    never enqueues on); runtimes beyond the budget are dealt as in the second case (profiles/stream_queues.md).
            // (PORESEQ_ONE_PRIORITY=1 forces the default level, PORESEQ_PRIORITY_LEVELS=1 the dealing.)
            auto make_stream = [&](hipStream_t* st) {
                static std::atomic<int> seq(0);
                const int mode = hwq_mode(nullptr);
                if (mode == 2 && private_stream(st, prop.multiProcessorCount)) return hipSuccess;
                const bool one = mode == 1;
                int lo = 0, hi = 0;
                if (!one && hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && lo > hi)
                    return hipStreamCreateWithPriority(st, hipStreamNonBlocking, hi + seq++ % (lo - hi + 1));
                return hipStreamCreateWithFlags(st, hipStreamNonBlocking);
            };
            if (hipSetDevice(dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess ||
                make_stream(&R.stream) != hipSuccess ||
                hipEventCreate(&R.ev0) != hipSuccess || hipEventCreate(&R.ev1) != hipSuccess ||
                hipEventCreate(&R.sw0) != hipSuccess || hipEventCreate(&R.sw1) != hipSuccess) {
                state = -1; why = "HIP device initialisation failed";
            } else if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos) {
                state = -1; why = std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only";
            } else {
                R.device = dev; R.ready = true; state = 1;
            }
        }
    }
    if (state < 0) return fail(PS_ERR_NO_DEVICE, why);
    if (R.stage.dirty) {   // a new API call: nothing staged by the previous one may still be in flight
        PS_HIP(hipStreamSynchronize(R.stream));
        if (R.stream2) PS_HIP(hipStreamSynchronize(R.stream2));
        PS_TRY(R.stage.reset());
    }
    *out = &R;
    return PS_OK;
}

static hipEvent_t prof_event(Runtime* rt) {
    hipEvent_t e = nullptr;
    if (!rt->prof_spare.empty()) { e = rt->prof_spare.back(); rt->prof_spare.pop_back(); }
    else if (hipEventCreate(&e) != hipSuccess) e = nullptr;
    return e;
}
void prof_begin(Runtime* rt) {
    if (!rt->prof_on) return;
    if (rt->prof_defer) {
        Runtime::ProfPend p{prof_event(rt), nullptr, nullptr, 0.0};
        if (p.a) (void)hipEventRecord(p.a, rt->stream);
        rt->prof_pend.push_back(p);
        return;
    }
    (void)hipEventRecord(rt->ev0, rt->stream);
}
void prof_end(Runtime* rt, const char* name, double bytes) {
    if (!rt->prof_on) return;
    if (rt->prof_defer) {
        if (rt->prof_pend.empty() || rt->prof_pend.back().b) return;
        Runtime::ProfPend& p = rt->prof_pend.back();
        p.b = prof_event(rt); p.name = name; p.bytes = bytes;   // (names are string literals)
        if (p.b) (void)hipEventRecord(p.b, rt->stream);
        return;
    }
    (void)hipEventRecord(rt->ev1, rt->stream);
    (void)hipEventSynchronize(rt->ev1);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, rt->ev0, rt->ev1);
    Prof& p = rt->prof[name];
    p.ms += ms; p.launches += 1; p.bytes += bytes;
}
// read the queued event pairs (deferred mode); the stream is drained first
void prof_flush(Runtime* rt) {
    if (rt->prof_pend.empty()) return;
    (void)hipStreamSynchronize(rt->stream);
    for (Runtime::ProfPend& q : rt->prof_pend) {
        float ms = 0;
        if (q.a && q.b && q.name && hipEventElapsedTime(&ms, q.a, q.b) == hipSuccess) {
            Prof& p = rt->prof[q.name];
            p.ms += ms; p.launches += 1; p.bytes += q.bytes;
        }
        if (q.a) rt->prof_spare.push_back(q.a);
        if (q.b) rt->prof_spare.push_back(q.b);
    }
    rt->prof_pend.clear();
}

// run fn(k) for k in [0, n) on the calling thread plus helpers from a process-wide pool of host threads (disjoint outputs; the GPU
// work of a batched call is enqueued by the caller).  The pool's threads live for the process: a lock-step schedule makes ~500 such
// calls per batch, fourteen batches at once — creating up to 32 threads for each of them cost more than most of the loops.  Helpers
// per call: PORESEQ_HOST_THREADS (poreseq_amd.dist.init sets it to this rank's share of the node's cores when several ranks share a
// node), else up to 32; the pool holds twice that for callers that overlap.  A helper that is dequeued after the caller and the
// other helpers have taken every index finds nothing to do and never touches the caller's frame.
namespace {
struct ParJob {
    std::function<void(int)> fn;
    int n = 0;
    std::atomic<int> next{0}, done{0};
    std::mutex mu;
    std::condition_variable cv;
    void run() {
        int did = 0;
        for (int k = next++; k < n; k = next++) { fn(k); did++; }
        if (did && (done += did) >= n) { std::lock_guard<std::mutex> lk(mu); cv.notify_all(); }
    }
};
struct ParPool {
    std::mutex mu;
    std::condition_variable cv;
    std::deque<std::shared_ptr<ParJob>> q;
    std::vector<std::thread> th;
    int idle = 0;
    size_t cap = 64;
    void worker() {
        std::unique_lock<std::mutex> lk(mu);
        for (;;) {
            idle++;
            cv.wait(lk, [&] { return !q.empty(); });
            idle--;
            std::shared_ptr<ParJob> j = q.front();
            q.pop_front();
            lk.unlock();
            j->run();
            j.reset();
            lk.lock();
        }
    }
    void submit(const std::shared_ptr<ParJob>& j, int helpers) {
        std::lock_guard<std::mutex> lk(mu);
        for (int k = 0; k < helpers; k++) q.push_back(j);
        int need = (int)q.size() - idle;   // queued tasks no waiting worker will take: new workers, up to the pool's size
        for (; need > 0 && th.size() < cap; need--) { th.emplace_back([this] { worker(); }); th.back().detach(); }
        cv.notify_all();
    }
};
static int par_cap() { static const int cap = [] { const char* e = getenv("PORESEQ_HOST_THREADS"); const int v = e ? atoi(e) : 32; return std::max(1, std::min(v, 64)); }(); return cap; }
ParPool* par_pool() {   // (never destroyed: its threads are detached and may outlive main; its size is set once, here)
    static ParPool* p = [] { ParPool* q = new ParPool(); q->cap = (size_t)std::max(2 * par_cap(), 8); return q; }();
    return p;
}
}  // namespace

void par_for(int n, const std::function<void(int)>& fn) {
    if (n <= 1) { if (n == 1) fn(0); return; }
    const int cap = par_cap();
    const int nth = std::min(n, cap);
    if (nth <= 1) { for (int k = 0; k < n; k++) fn(k); return; }
    std::shared_ptr<ParJob> j = std::make_shared<ParJob>();
    j->fn = fn; j->n = n;
    par_pool()->submit(j, nth - 1);
    j->run();
    std::unique_lock<std::mutex> lk(j->mu);
    j->cv.wait(lk, [&] { return j->done.load() >= n; });
}

// one line about the process-wide state of the library (ps_info): stream / hardware-queue mode, runtimes, memory plan
std::string info_string() {
    std::string why;
    if (hwq_mode(&why) == 2) {   // how many runtimes hold a private queue, how many were dealt a priority level instead
        const int held = g_pq_held.load(), fell = g_pq_fell.load();
        why += ": " + std::to_string(held) + " private (budget " + std::to_string(private_queue_budget()) + ") on one priority level, " +
               (fell ? std::to_string(fell) + " fell back and are dealt over the priority levels" : std::string("none fell back"));
    }
    const MemInfo m = mem_info();
    char buf[512];
    snprintf(buf, sizeof buf, "; device fraction of this process %.3f; runtimes: %d live, %d peak; share per runtime %.1f GB; slabs for full score matrices: %zu of %d allocated (%.1f GB, %.1f GB each by plan); device pools of this process %.1f GB",
             device_fraction(), live_runtimes(), peak_runtimes(), device_share_bytes() * 1e-9, m.slabs, m.slabs_planned, m.slab_bytes * 1e-9, slab_bytes() * 1e-9, (double)m.pool_bytes * 1e-9);
    return "hip-gfx950; streams: " + why + buf;
}

}  // namespace ps
