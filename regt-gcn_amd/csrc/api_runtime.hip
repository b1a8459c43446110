// Process and runtime state of the host layer: error text, per-device launch state, stage profiling, hipGraph replay, side streams, per-call flags.
#include <stdarg.h>

#include <map>
#include <string>

#include "api_internal.h"

namespace regt {

static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// ---- per-device launch state (kernels.h) ----------------------------------------------------------------------------
struct GraphStream { hipStream_t s = nullptr; hipEvent_t in = nullptr, out = nullptr; };
struct DeviceState {
    std::atomic<int> cus{0};
    GraphStream graph;        // capture / replay stream of run_maybe_graphed and its event pair (guarded by g_graph_stream_mu)
};
static DeviceState g_devices[MAX_DEVICES];

int current_device() {
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return -1; }
    return dev;
}
int device_cus(int dev) {
    const bool cached = (unsigned)dev < (unsigned)MAX_DEVICES;
    int cus = cached ? g_devices[dev].cus.load(std::memory_order_relaxed) : 0;
    if (cus > 0) return cus;
    if (dev < 0 || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) return 256;
    if (cached) g_devices[dev].cus.store(cus, std::memory_order_relaxed);
    return cus;
}
// (a slow, host-synchronous driver call: want_dynamic_lds makes it once per kernel and device)
int set_dynamic_lds(const void* kernel, int bytes) {
    REGT_CHECK_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    return REGT_OK;
}

// ---- optional per-kernel timing with HIP events (ProfScope) ------------------------------------------
bool g_prof_on = false;
std::vector<ProfRec> g_prof;
std::mutex g_prof_mu;

// ---- hipGraph replay for launch-bound problem sizes -------------------------------------------------------
// A forward or backward of a small graph (TPIMS: 104 nodes) is ~40-75 kernel launches of a few microseconds
// each.  Optionally (REGT_HIPGRAPH=1) the launch sequence of such sizes is captured
// into a hipGraph the SECOND time the same set of buffers is seen (pointers are the cache key: a graph is only
// ever replayed onto exactly the buffers it was captured with) and replayed from then on.
// Capture cannot run on the legacy default stream PyTorch uses, so graphs are captured and replayed on a
// library-owned stream of the current device that is ordered against the caller's stream with two events.
GraphCache g_fwd_graphs, g_bwd_graphs;
static const long GRAPH_MAX_ROWS = 1L << 15;   // N*T rows below which a step is launch-bound

unsigned long long hash_bytes(const void* p, size_t n, unsigned long long h) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 0x100000001B3ull; }
    return h;
}

// REGT_HIPGRAPH: 0 (default) off, 1 small problems only, 2 always.  Opt-in: measured 1.05 vs 0.89 ms/step at TPIMS size (the step
// is bound by the latency of many tiny dependent kernels, not by their launches)
bool graphs_wanted(long rows) {
    const int mode = option(OPT_HIPGRAPH);
    if (g_prof_on || mode == 0) return false;
    return mode == 2 || rows <= GRAPH_MAX_ROWS;
}

static std::mutex g_graph_stream_mu;   // a device's GraphStream is shared by the forward and backward caches
int run_maybe_graphed(GraphCache& cache, unsigned long long key, hipStream_t st, const std::function<int(hipStream_t)>& enqueue) {
    std::lock_guard<std::mutex> lk_stream(g_graph_stream_mu);
    std::lock_guard<std::mutex> lk(cache.mu);
    // a captured launch sequence is only valid for the arithmetic and on the device it was captured with
    const int gm_dev[2] = {gemm_mode(), current_device()};
    key = hash_bytes(gm_dev, sizeof(gm_dev), key);
    if ((unsigned)gm_dev[1] >= (unsigned)MAX_DEVICES) { ++cache.eager; return enqueue(st); }
    GraphStream& gs = g_devices[gm_dev[1]].graph;
    GraphEntry& e = cache.map[key];
    if (!e.exec) {
        if (e.seen++ == 0 || cache.map.size() > 256) {   // first sighting (the plain launches also raise the kernels' LDS limits
            ++cache.eager;                               // on this device), or buffers keep changing: plain launches
            return enqueue(st);
        }
        if (!gs.s) {
            REGT_CHECK_HIP(hipStreamCreateWithFlags(&gs.s, hipStreamNonBlocking));
            REGT_CHECK_HIP(hipEventCreateWithFlags(&gs.in, hipEventDisableTiming));
            REGT_CHECK_HIP(hipEventCreateWithFlags(&gs.out, hipEventDisableTiming));
        }
        hipGraph_t graph = nullptr;
        REGT_CHECK_HIP(hipStreamBeginCapture(gs.s, hipStreamCaptureModeRelaxed));
        const int rc = enqueue(gs.s);
        const hipError_t ce = hipStreamEndCapture(gs.s, &graph);
        if (rc != REGT_OK || ce != hipSuccess || !graph) {
            if (graph) (void)hipGraphDestroy(graph);
            (void)hipGetLastError();
            e.seen = -(1 << 30);                         // never try again for this key
            return rc != REGT_OK ? rc : enqueue(st);
        }
        const hipError_t ie = hipGraphInstantiate(&e.exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (ie != hipSuccess) { e.exec = nullptr; e.seen = -(1 << 30); (void)hipGetLastError(); return enqueue(st); }
        ++cache.captured;
    }
    ++cache.replayed;
    REGT_CHECK_HIP(hipEventRecord(gs.in, st));
    REGT_CHECK_HIP(hipStreamWaitEvent(gs.s, gs.in, 0));
    REGT_CHECK_HIP(hipGraphLaunch(e.exec, gs.s));
    REGT_CHECK_HIP(hipEventRecord(gs.out, gs.s));
    REGT_CHECK_HIP(hipStreamWaitEvent(st, gs.out, 0));
    return REGT_OK;
}

thread_local unsigned t_call_flags = 0;      // regt_dims.flags of the entry point running on this thread (CallScope)

// ---- side stream for work off the critical path of a backward pass -----------------------------------------------------------------
// The two weight gradients of the head (a few hundred MB of reads, grids far smaller than the chip) depend only on the head's own
// data gradient; the cell backward that follows on the launch stream does not need them.  They run on a library-owned stream,
// forked behind the kernel that produces d1 and joined in front of the slab reduction: 0.18 ms of the cfg-5 shard step (and
// of a one-region-per-GPU shard, where such fixed costs are what strong scaling loses) overlap the cell backward instead of
// preceding it.  REGT_SIDE_STREAM=0 keeps everything on the launch stream; captured launch sequences (REGT_HIPGRAPH) do too.
struct SideStream {
    hipStream_t s = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
    bool forked = false;
};
// One side stream (+ its event pair and fork state) per (device, launch stream): two launch streams, two devices or two host
// threads with streams of their own never share fork / join state.  (Two threads enqueueing on the SAME launch stream at once
// are the caller's race, as for any stream.)  The table is guarded by a mutex; HIP calls on the entry run under it, too -- they
// only enqueue.
static std::mutex g_side_mu;
static std::map<std::pair<int, hipStream_t>, SideStream> g_sides;
static const size_t SIDE_MAX_STREAMS = 64;
hipStream_t side_fork(hipStream_t st) {
    if (t_call_flags & REGT_DIMS_NO_SIDE_STREAM) return st;
    if (!option(OPT_SIDE_STREAM) || option(OPT_HIPGRAPH) > 0) return st;        // REGT_SIDE_STREAM=0; never inside a captured graph
    std::lock_guard<std::mutex> lk(g_side_mu);
    const int dev = current_device();
    if (dev < 0) return st;
    const auto key = std::make_pair(dev, st);
    auto it = g_sides.find(key);
    if (it == g_sides.end()) {
        if (g_sides.size() >= SIDE_MAX_STREAMS) return st;        // a caller cycling through many streams: stay on the launch stream
        SideStream ns;
        if (hipStreamCreateWithFlags(&ns.s, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&ns.fork, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&ns.join, hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            if (ns.s) (void)hipStreamDestroy(ns.s);
            if (ns.fork) (void)hipEventDestroy(ns.fork);
            return st;
        }
        it = g_sides.emplace(key, ns).first;
    }
    SideStream& ss = it->second;
    if (hipEventRecord(ss.fork, st) != hipSuccess || hipStreamWaitEvent(ss.s, ss.fork, 0) != hipSuccess) { (void)hipGetLastError(); return st; }
    ss.forked = true;
    return ss.s;
}
int side_join(hipStream_t st) {
    std::lock_guard<std::mutex> lk(g_side_mu);
    const int dev = current_device();
    if (dev < 0) return REGT_OK;
    auto it = g_sides.find(std::make_pair(dev, st));
    if (it == g_sides.end() || !it->second.forked) return REGT_OK;
    SideStream& ss = it->second;
    ss.forked = false;
    REGT_CHECK_HIP(hipEventRecord(ss.join, ss.s));
    REGT_CHECK_HIP(hipStreamWaitEvent(st, ss.join, 0));
    return REGT_OK;
}
// the side stream (if this launch stream has one in use) continues only after everything enqueued on `st` so far: used when a slab
// region is handed out again after an overflow flush -- the reduction that still reads it runs on `st`
void side_resync(hipStream_t st) {
    {
        std::lock_guard<std::mutex> lk(g_side_mu);
        const int dev = current_device();
        if (dev < 0 || g_sides.find(std::make_pair(dev, st)) == g_sides.end()) return;
    }
    (void)side_fork(st);
}

}  // namespace regt

using namespace regt;

extern "C" {

int32_t regt_abi_version(void) { return REGT_ABI_VERSION; }

int32_t regt_set_gemm_mode(int32_t mode) {
    const int prev = gemm_mode();       // (as the calling thread sees it)
    set_option(OPT_GEMM_MODE, mode);
    return prev;
}
int32_t regt_gemm_mode(void) { return gemm_mode(); }      // (as the calling thread sees it; reads only)
const char* regt_last_error(void) { return g_err; }

int32_t regt_set_option(const char* name, int32_t value) {
    REGT_CHECK_ARG(name != nullptr, "regt_set_option: name is NULL");
    return set_option(name, value);
}

/* out[0..5] = forward {eager, captured, replayed}, backward {eager, captured, replayed} launch-sequence counts */
int32_t regt_graph_stats(int64_t* out) {
    REGT_CHECK_ARG(out != nullptr, "regt_graph_stats: NULL pointer");
    out[0] = g_fwd_graphs.eager; out[1] = g_fwd_graphs.captured; out[2] = g_fwd_graphs.replayed;
    out[3] = g_bwd_graphs.eager; out[4] = g_bwd_graphs.captured; out[5] = g_bwd_graphs.replayed;
    return REGT_OK;
}

int64_t regt_debug_trace(int64_t* out_host, int64_t capacity) { return fused_trace_fetch(reinterpret_cast<long*>(out_host), (long)capacity); }

int32_t regt_profile_enable(int32_t on) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof_on = on != 0;
    return REGT_OK;
}

/* Waits for all recorded events, writes one line per stage "name count total_ms\n" into buf, clears the records. */
int32_t regt_profile_collect(char* buf, size_t buf_bytes) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    std::map<std::string, std::pair<long, double>> agg;
    for (auto& r : g_prof) {
        float ms = 0.f;
        if (hipEventSynchronize(r.e1) == hipSuccess && hipEventElapsedTime(&ms, r.e0, r.e1) == hipSuccess) {
            auto& a = agg[r.name];
            a.first += 1;
            a.second += ms;
        }
        (void)hipEventDestroy(r.e0);
        (void)hipEventDestroy(r.e1);
    }
    g_prof.clear();
    std::string out;
    char line[160];
    for (auto& kv : agg) {
        snprintf(line, sizeof(line), "%s %ld %.6f\n", kv.first.c_str(), kv.second.first, kv.second.second);
        out += line;
    }
    REGT_CHECK_ARG(buf && buf_bytes > out.size(), "regt_profile_collect: buffer too small (%zu needed)", out.size() + 1);
    memcpy(buf, out.c_str(), out.size() + 1);
    return REGT_OK;
}

}  // extern "C"
