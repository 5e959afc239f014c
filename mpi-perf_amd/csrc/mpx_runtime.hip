// mpx_runtime.hip — host side of libmpx: contexts, buffers, rank registration
// (same-process peer access or cross-process IPC), copy, the latency
// recorder and the C-ABI entry points.  The three transfer engines behind
// mpx_xfer_ex are in mpx_engine_kernel.hip (kernel; also mpx_xfer_arm and
// mpx_xfer_fan) and mpx_engine_stream.hip (SDMA, RCCL); what the parts share
// is declared in mpx_runtime.h.
//
// Reference mapping (all /root/reference/mpi_perf.c):
//   mpx_init/finalize        MPI_Init / MPI_Finalize              :372, :581
//   mpx_alloc/fill/free      allocate_tx_rx_buffers, free         :240-252, :574-578
//   mpx_rank_attach/export/import   get_peer_rank's node_info Allgather :200-238
//   mpx_xfer(_ex)            do_mpi_benchmark{,_nonblocking,_unidir} :66-145
//   mpx_barrier              MPI_Barrier                          :499, :557, :579
#include "mpx_runtime.h"
#include "mpx_seq.h"

using namespace mpx;

namespace {
thread_local std::string g_last_error;
}

namespace mpx {

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

std::atomic<int>& live_events() {
    static std::atomic<int> n{0};
    return n;
}

namespace {

struct RankDesc {
    char magic[8];
    int32_t abi, rank, dev, mb_kind;
    int64_t pid;
    uint64_t len;
    char bus_id[32];
    char host[64];
    hipIpcMemHandle_t rx_handle;
    hipIpcMemHandle_t mb_handle;
    uint64_t ring_bytes;
    hipIpcMemHandle_t ring_handle;   // valid when ring_bytes > 0
    hipIpcMemHandle_t tx_handle;     // the rank's tx: pull mode loads from it
};
static_assert(sizeof(RankDesc) <= MPX_RANK_DESC_BYTES, "rank descriptor too large");

int util_stream(mpx_ctx* ctx, int dev, hipStream_t* s) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    auto it = ctx->dev_stream.find(dev);
    if (it != ctx->dev_stream.end()) {
        *s = it->second;
        return MPX_OK;
    }
    DeviceGuard g(dev);
    HIPCK(g.err);
    hipStream_t st;
    HIPCK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    u64* tmp;
    // [0] checksum sum; [16 ..) the one-launch copies' barrier: 17 words
    // 128 B apart (top counter, 8 group counters, 8 release words)
    HIPCK(hipMalloc(&tmp, 16 * 19 * sizeof(u64)));
    ctx->dev_stream[dev] = st;
    ctx->dev_tmp[dev] = tmp;
    *s = st;
    return MPX_OK;
}

int check_dev(int dev) {
    int n = 0;
    HIPCK(hipGetDeviceCount(&n));
    if (dev < 0 || dev >= n) return fail(MPX_ERR_INVALID, "device %d out of range [0,%d)", dev, n);
    return MPX_OK;
}

// Allocate the rank's mailbox; prefer uncached device memory (every access
// goes to memory, so polls see xGMI stores), then fine-grained, then coarse.
// The kind must also be IPC-exportable for multi-process use.
int alloc_mailbox(Rank& rk) {
    const unsigned flags[2] = {hipDeviceMallocUncached, hipDeviceMallocFinegrained};
    for (int k = 0; k <= 1; ++k) {
        void* p = nullptr;
        if (hipExtMallocWithFlags(&p, sizeof(Mailbox), flags[k]) != hipSuccess) {
            (void)hipGetLastError();
            continue;
        }
        hipIpcMemHandle_t h;
        const hipError_t e = hipIpcGetMemHandle(&h, p);
        if (getenv("MPX_DEBUG"))
            fprintf(stderr, "[mpx] mailbox kind %d alloc ok, ipc handle: %s\n", k, hipGetErrorString(e));
        (void)hipGetLastError();
        if (e != hipSuccess) {
            (void)hipFree(p);
            continue;
        }
        rk.mb = static_cast<Mailbox*>(p);
        rk.mb_kind = k;
        return MPX_OK;
    }
    void* p = nullptr;
    HIPCK(hipMalloc(&p, sizeof(Mailbox)));
    if (getenv("MPX_DEBUG")) fprintf(stderr, "[mpx] mailbox kind 2 (coarse hipMalloc)\n");
    rk.mb = static_cast<Mailbox*>(p);
    rk.mb_kind = kMbCoarse;
    return MPX_OK;
}

}  // namespace

// Grows the checksum array without hipFree: hipFree waits for the whole
// device, i.e. for other ranks' spinning transfer kernels on the same GPU,
// which may be waiting for this rank.  Retired arrays are freed at finalize.
int ensure_csum(Rank& rk, int iters) {
    if ((size_t)iters <= rk.csum_cap) return MPX_OK;
    if (rk.csum) rk.retired.push_back(rk.csum);
    rk.csum = rk.cnt = nullptr;
    size_t cap = 1024;
    while (cap < (size_t)iters) cap *= 2;
    HIPCK(hipMalloc(&rk.csum, 2 * cap * sizeof(u64)));
    rk.cnt = rk.csum + cap;
    rk.csum_cap = cap;
    return MPX_OK;
}

namespace {

// Frees a local rank's device and host memory (rk.dev current, its stream
// drained): mpx_finalize, and release_rank on a failed attach.
void free_rank_memory(Rank& rk) {
    if (rk.mb) (void)hipFree(rk.mb);
    if (rk.ring) (void)hipFree(rk.ring);
    if (rk.scratch) (void)hipFree(rk.scratch);
    if (rk.csum) (void)hipFree(rk.csum);
    if (rk.lat.base) (void)hipFree(rk.lat.base);
    if (rk.fan_lat.base) (void)hipFree(rk.fan_lat.base);
    if (rk.hostlink_lat.base) (void)hipFree(rk.hostlink_lat.base);
    if (rk.fan_tab) (void)hipFree(rk.fan_tab);
    if (rk.fan_host) (void)hipHostFree(rk.fan_host);
    for (void* q : rk.retired) (void)hipFree(q);
    if (rk.status) (void)hipHostFree(rk.status);
}

// Bytes of a rank's check-mode receive ring: up to 255 further slots of the
// attached length, capped at MPX_CHECK_RING_BYTES (default 64 MiB; 0 = rx
// only, one slot per link).
uint64_t ring_bytes_for(size_t len) {
    static const uint64_t cap = [] {
        const char* v = getenv("MPX_CHECK_RING_BYTES");
        return v ? (uint64_t)strtoull(v, nullptr, 0) : (uint64_t)64 << 20;
    }();
    if (len == 0) return 0;
    const uint64_t want = (uint64_t)(kNbWindow - 1) * len;
    const uint64_t slots = (want < cap ? want : cap) / len;
    return slots * len;
}

// The check-mode receive ring of a local rank, allocated on its first use
// (a non-blocking call in check mode, by either rank of the link) or when the
// rank is exported: a peer process may push into it, and the descriptor
// carries its IPC handle.  A job that never checks non-blocking payloads
// never pays for it (up to 64 MiB per rank).  Caller holds ctx->mu.
int ensure_ring(Rank& rk) {
    if (!rk.local || rk.ring) return MPX_OK;
    const uint64_t bytes = ring_bytes_for(rk.len);
    if (!bytes) return MPX_OK;
    DeviceGuard g(rk.dev);
    HIPCK(g.err);
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, bytes);
    if (e == hipErrorOutOfMemory)
        return fail(MPX_ERR_NOMEM, "check ring of %llu B on device %d", (unsigned long long)bytes, rk.dev);
    HIPCK(e);
    rk.ring = static_cast<unsigned char*>(p);
    rk.ring_bytes = bytes;
    return MPX_OK;
}

// mpx_copy's form.  Default: all copies of a call in one launch where a
// launch per copy is dispatch-bound — k_copy_steps up to 512 KiB, k_copy_pipe
// above it to 16 MiB — and a k_copy launch per copy above.
// MPX_COPY (read per call; the tests drive every form and shape with it):
//   "launch"                      a k_copy launch per copy, any size
//   "steps[:cap:xcd:drain:upl:threads:one_xcd]"   k_copy_steps at any size
//   "pipe[:upl[:hier]]"           k_copy_pipe at any size it can hold
// MPX_COPY_WINDOW (read per call too): k_copy_win's resident window, see
// copy_window_parse (mpx_internal.h).
// Round 3's six copy knobs (MPX_COPY_VARIANT, _STEPS, _STEPS_MAX,
// _PIPE_MIN, _PIPE_MAX, _PIPE_UPL, _PIPE_HIER) are this one.
enum CopyForm { kCopyAuto = 0, kCopyLaunch, kCopySteps, kCopyPipe };
struct CopyChoice {
    int form = kCopyAuto;
    bool shaped = false;
    int shape[6] = {0, 0, 0, 0, 0, 0};   // k_copy_steps: cap, xcd, drain, upl, threads, one_xcd
    int upl = 0, hier = -1;              // k_copy_pipe
};
CopyChoice copy_choice() {
    CopyChoice c;
    const char* v = getenv("MPX_COPY");
    if (!v || !*v) return c;
    if (!strncmp(v, "launch", 6)) {
        c.form = kCopyLaunch;
    } else if (!strncmp(v, "steps", 5)) {
        c.form = kCopySteps;
        int* x = c.shape;
        const int k = sscanf(v + 5, ":%d:%d:%d:%d:%d:%d", &x[0], &x[1], &x[2], &x[3], &x[4], &x[5]);
        c.shaped = k >= 5;   // one_xcd may be omitted (0)
    } else if (!strncmp(v, "pipe", 4)) {
        c.form = kCopyPipe;
        (void)sscanf(v + 4, ":%d:%d", &c.upl, &c.hier);
    }
    return c;
}

// Fault injection for the tests' negative controls, all in ONE variable:
//   MPX_TEST="skip_push=k,lag_wg=rank:wg:us,no_posted,no_pull_wait"
//   skip_push=k     the k-th push of every call (1-based) moves no payload
//                   bytes but is still signalled: a correct receiver's check
//                   must fail
//   lag_wg=r:w:us   in non-blocking check mode, workgroup w of rank r (w < 0
//                   counts from the last) stalls `us` before it checks the
//                   call's last receive (pull mode: before it loads the call's
//                   last payload), so that rank's call ends long after its peer's;
//                   in an MPX_FAN_LL call, link workgroup w of rank r stalls
//                   between its push and its wait of iteration iters / 2
//   no_posted       no receive-posted handshake (round 2's behaviour): the
//                   negative control of tests/test_gpu_ordering.py
//   no_pull_wait    pull mode: a sending side returns without waiting for the
//                   peer's loads of its tx (the buffer-reuse negative control)
//   host_lag=i:us   a host endpoint busy-waits `us` before its first step of
//                   iteration i of every ping-pong or unidir call (mpx_host_xfer):
//                   the stalled iteration both ends' host-link recorders must find
//   seq_stale=k     the k-th send (1-based) of every sequenced host-link call
//                   of a host endpoint (mpx_host_xfer_seq) repeats the payload
//                   of the send before it: a bulk send leaves tx unwritten, an
//                   LL send packs the key of iteration k - 2; for k = 1 it sends
//                   what tx held.  The GPU side's check must fail at exactly
//                   iteration k - 1 — the negative control of "every pulled
//                   payload is fresh"
//   fail_launch=r   rank r's kernel-engine calls fail before their kernel is
//                   enqueued (after take_numbers took their numbers): the
//                   rollback test of give_back (mpx_engine_kernel.hip)
//   fail_copy       mpx_copy fails after its events are created and the start
//                   one is recorded: the event-leak test (mpx_live_events)
// Whether the variable exists is read ONCE per process: a process that
// starts without it (bench.py, mpx_perf) never looks again, and none of the
// knobs can reach it.  The tests set it (empty) before their first call
// (tests/conftest.py) and change its value between calls.  The same gate
// (test_gate) guards mpx_test_advance_link.
bool test_gate() {
    static const bool gate = getenv("MPX_TEST") != nullptr;
    return gate;
}

}  // namespace

TestKnobs test_knobs() {
    TestKnobs k;
    if (!test_gate()) return k;
    const char* v = getenv("MPX_TEST");
    if (!v) return k;
    std::string all(v);
    size_t pos = 0;
    while (pos <= all.size()) {
        size_t end = all.find(',', pos);
        if (end == std::string::npos) end = all.size();
        const std::string item = all.substr(pos, end - pos);
        if (!item.compare(0, 10, "skip_push=")) k.skip_push = atoi(item.c_str() + 10);
        else if (!item.compare(0, 7, "lag_wg=")) {
            if (sscanf(item.c_str() + 7, "%d:%d:%lld", &k.lag_rank, &k.lag_wg, &k.lag_us) != 3) k.lag_rank = -1;
        } else if (item == "no_posted") k.no_posted = true;
        else if (item == "no_pull_wait") k.no_pull_wait = true;
        else if (!item.compare(0, 9, "host_lag=")) {
            if (sscanf(item.c_str() + 9, "%d:%lld", &k.host_lag_iter, &k.host_lag_us) != 2) k.host_lag_iter = -1;
        }
        else if (!item.compare(0, 10, "seq_stale=")) k.seq_stale = atoi(item.c_str() + 10);
        else if (!item.compare(0, 12, "fail_launch=")) k.fail_launch = atoi(item.c_str() + 12);
        else if (item == "fail_copy") k.fail_copy = true;
        pos = end + 1;
    }
    return k;
}

namespace {

// A rank's stream must own its hardware queue.  The two halves of a pair
// are co-dependent persistent kernels; when both ranks live on one GPU and
// HIP multiplexes their streams onto one of its GPU_MAX_HW_QUEUES shared
// queues, the second kernel waits behind the first and both time out.  A
// stream created with a CU mask is never placed on a shared queue, so every
// rank stream is created with a mask that enables all CUs.
//
// Teardown rule (gfx950 / ROCm 7.2, isolated with tools/stream_teardown.hip,
// profiles/r02_stream_teardown.txt): a CU-masked stream owns a dedicated HSA
// queue that hipStreamDestroy frees.  hipFree of memory whose last use was a
// kernel on such a destroyed stream leaves the runtime waiting on that queue:
// the next queue creation, stream destruction or the process exit hangs
// ("a0 m0 k0.0 d0 f0" hangs at exit; "a0 m0 k0.0 f0 d0" is fine; freeing a
// buffer no kernel touched is fine either way).  The other stalls of rounds
// 2-4 — in a later context of the -m gpu suite when each finalize destroyed
// its streams (profiles/r02_stream_destroy_suite_hang.txt,
// r03_pytest_nopool.log) and at exit in processes mode
// (r04_procs_exit_stall.txt) — were one race, root-caused in round 5 from
// the stacks (profiles/r05_exit_stall_symbolized.txt): the destroy dropped
// its reference before HIP's completion handler of the stream's last
// command did, and the queue was then destroyed on the HSA events thread,
// which deadlocked on itself.  callback_fence now closes it
// (event_thread_barrier).  Rank streams stay process-lifetime objects all
// the same — a CU-masked queue costs a KFD queue creation — : mpx_finalize
// drains them (callback_fence), frees every allocation of the context, and
// returns them to a per-device pool that later contexts reuse; the host
// destroys them with mpx_shutdown once no context is alive (mpx_perf in
// both modes, bench.py).  A host that never calls it leaves them to the
// runtime's exit teardown (every allocation their kernels touched is freed by
// then: the safe order).
struct StreamPool {
    std::mutex mu;
    std::map<int, std::vector<hipStream_t>> idle;    // per device
    std::vector<std::pair<int, hipStream_t>> all;    // every stream ever created
    int live_contexts = 0;
};
StreamPool& pool() {
    static StreamPool* p = new StreamPool;   // never destroyed: no static-destructor ordering
    return *p;
}

void fence_cb(void* p) { static_cast<std::atomic<int>*>(p)->fetch_add(1, std::memory_order_release); }

// Hands off twice through the HSA async-events thread, the one thread that
// runs every hsa_amd_signal_async_handler callback, serially (hsa_ext_amd.h)
// — HIP's command-completion handlers, which run host functions, among them.
// When the second hand-off has run, every handler whose signal was satisfied
// before the first was registered has returned (one pass of the events loop
// fires every satisfied signal, in an arbitrary order: hence two).  One
// signal serves the process (value 0, condition EQ 0: satisfied at once;
// each registration returns false and is dropped).  Bounded at 10 s like the
// fence; false if the thread never came round.
bool on_events_thread(hsa_signal_value_t, void* arg) {
    static_cast<std::atomic<int>*>(arg)->store(1, std::memory_order_release);
    return false;
}

bool event_thread_barrier() {
    static hsa_signal_t sig = [] {
        hsa_signal_t s{0};
        if (hsa_signal_create(0, 0, nullptr, &s) != HSA_STATUS_SUCCESS) s.handle = 0;
        return s;
    }();
    if (!sig.handle) return false;
    const double t_end = now_s() + 10.0;
    for (int k = 0; k < 2; ++k) {
        // heap-held: leaked if the bound expires, so a late handler never
        // writes a dead stack frame
        std::atomic<int>* done = new std::atomic<int>(0);
        if (hsa_amd_signal_async_handler(sig, HSA_SIGNAL_CONDITION_EQ, 0, on_events_thread, done) != HSA_STATUS_SUCCESS) {
            delete done;
            return false;
        }
        while (!done->load(std::memory_order_acquire) && now_s() < t_end) usleep(20);
        if (!done->load(std::memory_order_acquire)) return false;
        delete done;
    }
    return true;
}

// Before streams are destroyed (and before the memory their commands used is
// freed).  Why (round 5, symbolized from profiles/r04_procs_exit_stall.txt;
// DESIGN.md §5 "Exit"): HIP's completion handler of a stream's command runs
// on the HSA async-events thread and holds a reference to the stream's
// virtual device until it returns — after the host function it ran.  When
// hipStreamDestroy drops the stream's own reference first, the handler's
// release is the last one: ~VirtualGPU runs ON the events thread, takes the
// device's virtual-GPU lock, and for a CU-masked stream (never pooled)
// hsa_queue_destroy's AqlQueue destructor waits, with no timeout, in the KFD
// event wait (AMDKFD_IOC_WAIT_EVENTS) for the queue's inactive-signal
// handler — which only that same thread can run.  The thread never returns;
// the next runtime call that needs the lock (a later stream teardown, or the
// fat-binary unregistration at exit) waits forever.  hipStreamSynchronize
// and the host functions below cannot close that window: they return when the
// command completed or the host function ran, both BEFORE the handler's
// release.  So: two host functions go onto each stream as its last commands
// (every callback before the second has returned once it runs), the streams
// are drained, and then event_thread_barrier() waits until the events
// thread has come round twice, i.e. has left the handler that ran the second
// host function and dropped its reference.  After that the caller's
// hipStreamDestroy drops the last reference on its own thread.
// Repro without libmpx: tools/exit_stall_repro cycle_fence|cycle_barrier
// (profiles/r05_stream_teardown_cycles.jsonl).  The waits are bounded (10 s)
// only so that a runtime that never runs the callbacks cannot hang the
// caller; the order, not the time, is what the fence relies on.  Returns
// false when a bound expired (the caller then must not destroy the streams).
bool callback_fence(const std::vector<std::pair<int, hipStream_t>>& ss) {
    // heap-held counters: leaked if the bound expires, so a late callback
    // never writes freed memory
    std::atomic<int>* cnt = new std::atomic<int>[ss.size() ? ss.size() : 1];
    std::vector<bool> armed(ss.size(), false);
    int prev = -1;
    (void)hipGetDevice(&prev);
    for (size_t i = 0; i < ss.size(); ++i) {
        cnt[i].store(0);
        (void)hipSetDevice(ss[i].first);
        armed[i] = hipLaunchHostFunc(ss[i].second, fence_cb, &cnt[i]) == hipSuccess &&
                   hipLaunchHostFunc(ss[i].second, fence_cb, &cnt[i]) == hipSuccess;
        (void)hipGetLastError();
    }
    const double t_end = now_s() + 10.0;
    bool done = true;
    for (size_t i = 0; i < ss.size(); ++i) {
        while (armed[i] && cnt[i].load(std::memory_order_acquire) < 2 && now_s() < t_end) usleep(50);
        done &= !armed[i] || cnt[i].load(std::memory_order_acquire) >= 2;
        (void)hipSetDevice(ss[i].first);
        (void)hipStreamSynchronize(ss[i].second);
    }
    if (prev >= 0) (void)hipSetDevice(prev);
    if (done) delete[] cnt;
    else if (getenv("MPX_DEBUG")) fprintf(stderr, "[mpx] callback fence: host functions did not run in 10 s\n");
    const bool handed_off = event_thread_barrier();
    if (!handed_off && getenv("MPX_DEBUG")) fprintf(stderr, "[mpx] callback fence: events-thread barrier did not complete\n");
    return done && handed_off;
}

// A rank stream goes back to the pool at finalize; later contexts reuse it
// (a CU-masked queue costs a KFD queue creation).  Pooled streams are
// destroyed only by mpx_shutdown, once no context is alive — which may be
// mid-process (mpx.h; tests/test_gpu_teardown.py): callback_fence and its
// event_thread_barrier order that destroy after every completion handler's
// release (round 5's root cause of the stalls rounds 2-4 saw, when each
// finalize destroyed its streams, profiles/r03_pytest_nopool.log).
void release_rank_stream(int dev, hipStream_t s) {
    std::lock_guard<std::mutex> lk(pool().mu);
    pool().idle[dev].push_back(s);
}

int create_rank_stream(int dev, hipStream_t* s) {
    {
        std::lock_guard<std::mutex> lk(pool().mu);
        auto& v = pool().idle[dev];
        if (!v.empty()) {
            *s = v.back();
            v.pop_back();
            return MPX_OK;
        }
    }
    hipDeviceProp_t prop;
    HIPCK(hipGetDeviceProperties(&prop, dev));
    const int words = (prop.multiProcessorCount + 31) / 32;
    std::vector<uint32_t> mask((size_t)words, 0xffffffffu);
    HIPCK(hipExtStreamCreateWithCUMask(s, (uint32_t)words, mask.data()));
    std::lock_guard<std::mutex> lk(pool().mu);
    pool().all.emplace_back(dev, *s);
    return MPX_OK;
}

}  // namespace

// Non-blocking mode: a push is published (kernel engine: drained + flag;
// SDMA engine: flag kernel) every nb_publish() pushes and at the last one —
// receivers wait only at window flushes and at the end.
// MPX_NB_PUBLISH=k (a divisor of 256; 1 = every push).
int nb_publish() {
    static const int k = [] {
        const char* v = getenv("MPX_NB_PUBLISH");
        const int x = v ? atoi(v) : 16;
        return (x >= 1 && x <= kNbWindow && (kNbWindow % x) == 0) ? x : 16;
    }();
    return k;
}

// Pull mode (MPX_XFER_PULL): the call's flag, else MPX_XFER_PULL=1 in the
// environment (every rank of a job inherits it, so both sides agree).  Kernel
// engine only.
bool pull_requested(const mpx_xfer_opts* o) {
    static const bool env_pull = [] {
        const char* v = getenv("MPX_XFER_PULL");
        return v && atoi(v) != 0;
    }();
    return (o && (o->flags & MPX_XFER_PULL)) || env_pull;
}

// Pull mode loads from the peer's tx: an imported rank's tx is mapped here on
// first use (under the context lock: both halves of a pair, or several local
// ranks, may get here at once), on the device imports are opened on.
int ensure_peer_tx(mpx_ctx* ctx, Rank& peer, int peer_rank) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    return ensure_peer_tx_locked(ctx, peer, peer_rank);
}
int ensure_peer_tx_locked(mpx_ctx* ctx, Rank& peer, int peer_rank) {
    if (peer.tx) return MPX_OK;
    if (!peer.imported || !peer.tx_handle_valid)
        return fail(MPX_ERR_STATE, "pull mode: rank %d's tx is not known here", peer_rank);
    DeviceGuard g(ctx->import_dev);
    HIPCK(g.err);
    void* p = nullptr;
    const hipError_t e = hipIpcOpenMemHandle(&p, peer.tx_handle, hipIpcMemLazyEnablePeerAccess);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(MPX_ERR_HIP, "pull mode: mapping rank %d's tx: %s", peer_rank, hipGetErrorString(e));
    }
    ctx->ipc_opened.push_back(p);
    peer.tx = static_cast<unsigned char*>(p);
    return MPX_OK;
}

}  // namespace mpx

// ===========================================================================
// C-ABI
// ===========================================================================
extern "C" {

int mpx_version(void) { return MPX_ABI_VERSION; }

const char* mpx_strerror(int s) {
    switch (s) {
        case MPX_OK: return "success";
        case MPX_ERR_INVALID: return "invalid argument";
        case MPX_ERR_HIP: return "HIP runtime error";
        case MPX_ERR_NOMEM: return "out of device memory";
        case MPX_ERR_TIMEOUT: return "device-side wait timed out";
        case MPX_ERR_RCCL: return "RCCL error";
        case MPX_ERR_UNSUPPORTED: return "unsupported engine/mode";
        case MPX_ERR_STATE: return "call out of order";
        case MPX_ERR_CHECK: return "payload checksum mismatch";
        default: return "unknown mpx status";
    }
}

const char* mpx_last_error(void) { return g_last_error.c_str(); }

int mpx_device_count(int* count) {
    if (!count) return fail(MPX_ERR_INVALID, "count is NULL");
    HIPCK(hipGetDeviceCount(count));
    return MPX_OK;
}

int mpx_link_info(int dev_a, int dev_b, int* link_type, int* hops) {
    if (!link_type || !hops) return fail(MPX_ERR_INVALID, "NULL argument");
    TRY(check_dev(dev_a));
    TRY(check_dev(dev_b));
    if (dev_a == dev_b) return fail(MPX_ERR_INVALID, "device %d is both ends of the link", dev_a);
    uint32_t t = 0, h = 0;
    HIPCK(hipExtGetLinkTypeAndHopCount(dev_a, dev_b, &t, &h));
    *link_type = (int)t;
    *hops = (int)h;
    return MPX_OK;
}

int mpx_device_bus_id(int dev, char* buf, int len) {
    if (!buf || len < 16) return fail(MPX_ERR_INVALID, "bus id buffer too small");
    TRY(check_dev(dev));
    HIPCK(hipDeviceGetPCIBusId(buf, len, dev));
    return MPX_OK;
}

int mpx_init(int nranks, int engine, mpx_ctx** out) {
    if (!out) return fail(MPX_ERR_INVALID, "ctx out-pointer is NULL");
    *out = nullptr;
    if (nranks < 1 || nranks > MPX_MAX_RANKS) return fail(MPX_ERR_INVALID, "nranks %d not in [1,%d]", nranks, MPX_MAX_RANKS);
    if (engine == MPX_ENGINE_HOST)
        return fail(MPX_ERR_UNSUPPORTED, "engine HOST is not built: the CPU baseline is the compiled reference "
                    "(DESIGN.md section 8)");
    if (engine < MPX_ENGINE_KERNEL || engine > MPX_ENGINE_RCCL) return fail(MPX_ERR_INVALID, "engine %d", engine);
    int ndev = 0;
    HIPCK(hipGetDeviceCount(&ndev));
    if (ndev < 1) return fail(MPX_ERR_HIP, "no GPU visible");
    mpx_ctx* c = new mpx_ctx;
    c->nranks = nranks;
    c->engine = engine;
    {
        std::lock_guard<std::mutex> lk(pool().mu);
        ++pool().live_contexts;
    }
    *out = c;
    return MPX_OK;
}

#define DBG(...) \
    do { if (getenv("MPX_DEBUG")) { fprintf(stderr, "[mpx] " __VA_ARGS__); fflush(stderr); } } while (0)

int mpx_finalize(mpx_ctx* ctx) {
    if (!ctx) return fail(MPX_ERR_INVALID, "ctx is NULL");
    // Teardown order matters: every stream is drained and every allocation
    // freed, then the rank streams go back to the process pool (the teardown
    // rule above create_rank_stream).
    // Every stream of the context, rank and utility streams alike, is
    // drained through callback_fence: no completion callback of any of them
    // is still running when their memory is freed and the utility streams
    // are destroyed (a utility stream destroyed right after its drain stalled
    // mpx_perf at exit once the rank streams were fenced: r03_exit_hang).
    std::vector<std::pair<int, hipStream_t>> ss;
    for (int i = 0; i < MPX_MAX_RANKS; ++i) {
        Rank& rk = ctx->r[i];
        if (rk.armed) {                 // an armed call never started: cancel it
            DeviceGuard g(rk.dev);
            (void)disarm(rk);
        }
        if (rk.comm) (void)rccl_api().CommDestroy(rk.comm);
        rk.comm = nullptr;
        if (rk.local && rk.stream) ss.emplace_back(rk.dev, rk.stream);
    }
    for (auto& kv : ctx->dev_stream) ss.emplace_back(kv.first, kv.second);
    const bool fenced = callback_fence(ss);
    DBG("finalize: streams drained\n");
    for (int i = 0; i < MPX_MAX_RANKS; ++i) {
        for (auto& kv : ctx->r[i].sdma_graphs) (void)hipGraphExecDestroy(kv.second);
        ctx->r[i].sdma_graphs.clear();
    }
    for (void* p : ctx->ipc_opened) {
        const hipError_t e = hipIpcCloseMemHandle(p);
        if (e != hipSuccess) DBG("finalize: hipIpcCloseMemHandle(%p): %s\n", p, hipGetErrorString(e));
    }
    (void)hipGetLastError();
    for (int i = 0; i < MPX_MAX_RANKS; ++i) {
        Rank& rk = ctx->r[i];
        if (rk.host) free_host_endpoint(rk);
        if (!rk.local) continue;
        DeviceGuard g(rk.dev);
        free_rank_memory(rk);
    }
    for (auto& kv : ctx->allocs) {
        DeviceGuard g(kv.second.dev);
        (void)hipFree(reinterpret_cast<void*>(kv.first));
    }
    for (auto& kv : ctx->dev_tmp) {
        DeviceGuard g(kv.first);
        (void)hipFree(kv.second);
    }
    DBG("finalize: memory freed\n");
    for (int i = 0; i < MPX_MAX_RANKS; ++i) {
        Rank& rk = ctx->r[i];
        if (!rk.local) continue;
        DeviceGuard g(rk.dev);
        rk.ev0.reset();
        rk.ev1.reset();
        if (rk.stream) release_rank_stream(rk.dev, rk.stream);
    }
    if (fenced) {   // else left to the runtime: a destroy could be the events thread's last release
        for (auto& kv : ctx->dev_stream) {
            DeviceGuard g(kv.first);
            (void)hipStreamDestroy(kv.second);
        }
    }
    DBG("finalize: done\n");
    delete ctx;
    {
        std::lock_guard<std::mutex> lk(pool().mu);
        --pool().live_contexts;
    }
    return MPX_OK;
}

int mpx_alloc(mpx_ctx* ctx, int dev, size_t bytes, void** ptr) {
    if (!ctx || !ptr) return fail(MPX_ERR_INVALID, "NULL argument");
    *ptr = nullptr;
    TRY(check_dev(dev));
    DeviceGuard g(dev);
    HIPCK(g.err);
    void* p = nullptr;
    // hipMalloc returns >= 4 KiB-aligned blocks (posix_memalign(4096), mpi_perf.c:242-243)
    const hipError_t e = hipMalloc(&p, bytes ? bytes : 16);
    if (e == hipErrorOutOfMemory) return fail(MPX_ERR_NOMEM, "hipMalloc(%zu) on device %d", bytes, dev);
    HIPCK(e);
    if (reinterpret_cast<uintptr_t>(p) & 4095) {
        (void)hipFree(p);
        return fail(MPX_ERR_HIP, "hipMalloc returned a pointer that is not 4 KiB aligned");
    }
    // -b 0: the unidir ack still sends tx[0] (mpi_perf.c:142) out of a 0-byte
    // posix_memalign block — glibc hands back a fresh zeroed chunk, so the
    // reference's ack byte is 0 (its PMPI digest, tests/test_integration.py);
    // the 16-byte pad is zeroed to match, on the utility stream (the null
    // stream would wait for other ranks' persistent kernels)
    if (!bytes) {
        hipStream_t us = nullptr;
        const int st = util_stream(ctx, dev, &us);
        hipError_t z = hipSuccess;
        if (st == MPX_OK) {
            std::lock_guard<std::mutex> ul(ctx->util_mu);
            z = hipMemsetAsync(p, 0, 16, us);
            if (z == hipSuccess) z = hipStreamSynchronize(us);
        }
        if (st != MPX_OK || z != hipSuccess) {
            (void)hipFree(p);
            if (st != MPX_OK) return st;
            HIPCK(z);
        }
    }
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->allocs[reinterpret_cast<uintptr_t>(p)] = AllocRec{dev, bytes};
    *ptr = p;
    return MPX_OK;
}

int mpx_free(mpx_ctx* ctx, void* ptr) {
    if (!ctx) return fail(MPX_ERR_INVALID, "ctx is NULL");
    if (!ptr) return MPX_OK;
    AllocRec rec;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        auto it = ctx->allocs.find(reinterpret_cast<uintptr_t>(ptr));
        if (it == ctx->allocs.end()) return fail(MPX_ERR_INVALID, "%p was not allocated by mpx_alloc", ptr);
        rec = it->second;
        ctx->allocs.erase(it);
    }
    DeviceGuard g(rec.dev);
    HIPCK(hipFree(ptr));
    return MPX_OK;
}

int mpx_fill(mpx_ctx* ctx, int dev, void* ptr, size_t n, int pattern, uint64_t arg) {
    if (!ctx || (!ptr && n)) return fail(MPX_ERR_INVALID, "NULL argument");
    if (pattern != MPX_FILL_BYTE && pattern != MPX_FILL_SPLITMIX) return fail(MPX_ERR_INVALID, "pattern %d", pattern);
    if (n && (reinterpret_cast<uintptr_t>(ptr) & 7)) return fail(MPX_ERR_INVALID, "fill buffer must be 8-byte aligned");
    TRY(check_dev(dev));
    if (!n) return MPX_OK;
    hipStream_t s;
    TRY(util_stream(ctx, dev, &s));
    std::lock_guard<std::mutex> ul(ctx->util_mu);
    DeviceGuard g(dev);
    HIPCK(launch_fill(ptr, n, pattern, arg, s));
    HIPCK(hipStreamSynchronize(s));
    return MPX_OK;
}

int mpx_checksum(mpx_ctx* ctx, int dev, const void* ptr, size_t n, uint64_t* out) {
    if (!ctx || !out || (!ptr && n)) return fail(MPX_ERR_INVALID, "NULL argument");
    if (n && (reinterpret_cast<uintptr_t>(ptr) & 15))
        return fail(MPX_ERR_INVALID, "checksum buffer must be 16-byte aligned");
    TRY(check_dev(dev));
    hipStream_t s;
    TRY(util_stream(ctx, dev, &s));
    std::lock_guard<std::mutex> ul(ctx->util_mu);
    u64* tmp = ctx->dev_tmp[dev];
    DeviceGuard g(dev);
    u64 raw = 0;
    if (n) {
        HIPCK(hipMemsetAsync(tmp, 0, sizeof(u64), s));
        HIPCK(launch_checksum(ptr, n, tmp, s));
        HIPCK(hipMemcpyAsync(&raw, tmp, sizeof(u64), hipMemcpyDeviceToHost, s));
        HIPCK(hipStreamSynchronize(s));
    }
    *out = raw ^ mix64_host((u64)n);
    return MPX_OK;
}

int mpx_read(mpx_ctx* ctx, int dev, void* host_dst, const void* dev_src, size_t n) {
    if (!ctx || ((!host_dst || !dev_src) && n)) return fail(MPX_ERR_INVALID, "NULL argument");
    TRY(check_dev(dev));
    if (!n) return MPX_OK;
    hipStream_t s;
    TRY(util_stream(ctx, dev, &s));
    std::lock_guard<std::mutex> ul(ctx->util_mu);
    DeviceGuard g(dev);
    HIPCK(hipMemcpyAsync(host_dst, dev_src, n, hipMemcpyDeviceToHost, s));
    HIPCK(hipStreamSynchronize(s));
    return MPX_OK;
}

int mpx_copy(mpx_ctx* ctx, int dev, void* dst, const void* src, size_t n, int iters, mpx_timing* t) {
    if (!ctx || !t || ((!dst || !src) && n) || iters < 0) return fail(MPX_ERR_INVALID, "bad argument");
    if ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 15)
        return fail(MPX_ERR_INVALID, "copy buffers must be 16-byte aligned");
    TRY(check_dev(dev));
    memset(t, 0, sizeof *t);
    hipStream_t s;
    TRY(util_stream(ctx, dev, &s));
    std::lock_guard<std::mutex> ul(ctx->util_mu);
    DeviceGuard g(dev);
    Event e0, e1;   // destroyed on every return below
    HIPCK(e0.create());
    HIPCK(e1.create());
    int grid = 0;
    // All iterations in one launch where a launch per copy is dispatch-bound:
    // k_copy_pipe above 512 KiB to 16 MiB, k_copy_steps up to 512 KiB; one
    // k_copy launch per copy above (profiles/r03_copy_pipe_ab.jsonl, DESIGN.md
    // §5) — or the form MPX_COPY forces (copy_choice)
    const CopyChoice cc = copy_choice();
    // a launch per copy: which blocks of src stay in the Infinity Cache for the
    // next copy (copy_window_rule, or the window MPX_COPY_WINDOW forces)
    CopyWindow win;
    if (!copy_window_parse(getenv("MPX_COPY_WINDOW"), n, &win))
        return fail(MPX_ERR_INVALID, "MPX_COPY_WINDOW is not \"period:window[:unit]\" (multiples of 4096, "
                                     "period / 4096 and unit / 4096 powers of two, window <= period) or \"0\"");
    const bool multi = n && iters > 1;
    bool pipe = multi && (cc.form == kCopyPipe ||
                          (cc.form == kCopyAuto && n > kCopyPipeDefaultMin && n <= kCopyPipeDefaultMax));
    const bool steps = multi && !pipe && (cc.form == kCopySteps || (cc.form == kCopyAuto && n <= kCopyPipeDefaultMin));
    bool one = pipe || steps;          // all copies in one launch
    u64* bar = ctx->dev_tmp[dev] + 16;
    float ms = 0;
    double t0 = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
        if (one) HIPCK(hipMemsetAsync(bar, 0, 17 * 16 * sizeof(u64), s));   // top + 8 group counters + 8 release words
        t0 = now_s();
        HIPCK(hipEventRecord(e0, s));
        if (test_knobs().fail_copy) return fail(MPX_ERR_HIP, "copy failed after its start event (MPX_TEST fail_copy)");
        if (one && pipe) {
            const hipError_t e = launch_copy_pipe(dst, src, n, iters, bar, s, &grid, cc.upl, cc.hier);
            if (e == hipErrorInvalidValue) {
                // too large for a resident pipe grid (a forced form or shape):
                // a launch per copy instead
                (void)hipGetLastError();
                one = pipe = false;
                continue;
            }
            HIPCK(e);
        } else if (one)
            HIPCK(launch_copy_steps(dst, src, n, iters, bar, s, &grid, cc.shaped ? cc.shape : nullptr));
        else
            for (int i = 0; i < iters && n; ++i) HIPCK(launch_copy(dst, src, n, s, &grid, win));
        HIPCK(hipEventRecord(e1, s));
        HIPCK(hipEventSynchronize(e1));
        HIPCK(hipEventElapsedTime(&ms, e0, e1));
        if (!one) break;
        // k_copy_steps / k_copy_pipe gave up on its grid barrier (bar[1]):
        // not every workgroup became resident — e.g. other ranks' persistent
        // transfer kernels hold CUs of this GPU.  Copy again, a launch per copy
        // (no residency needed); that is the call's result and its time.
        u64 stop = 0;
        HIPCK(hipMemcpyAsync(&stop, bar + 1, sizeof stop, hipMemcpyDeviceToHost, s));
        HIPCK(hipStreamSynchronize(s));
        if (!stop) break;
        DBG("copy of %zu B: step barrier gave up, a launch per copy instead\n", n);
        one = false;
    }
    t->wall_s = now_s() - t0;
    t->device_s = ms * 1e-3;
    t->bytes = (uint64_t)n * (uint64_t)iters;
    t->launches = !n ? 0 : one ? 1 : iters;
    t->nwg = grid;
    t->protocol = !one ? kProtoCopy : pipe ? kProtoCopyPipe : kProtoCopySteps;
    return MPX_OK;
}

namespace {

// A local rank's own resources: mailbox, stream, events, status, scratch,
// checksum arrays and the check-mode receive ring (rk.dev current).
int attach_resources(Rank& rk) {
    HIPCK(hipDeviceGetPCIBusId(rk.bus_id, sizeof rk.bus_id, rk.dev));
    TRY(alloc_mailbox(rk));
    TRY(create_rank_stream(rk.dev, &rk.stream));
    HIPCK(hipMemsetAsync(rk.mb, 0, sizeof(Mailbox), rk.stream));
    HIPCK(rk.ev0.create());
    HIPCK(rk.ev1.create());
    HIPCK(hipHostMalloc(reinterpret_cast<void**>(&rk.status), sizeof(Status), hipHostMallocCoherent | hipHostMallocMapped));
    memset(rk.status, 0, sizeof(Status));
    HIPCK(hipMalloc(&rk.scratch, kScratchWords * sizeof(u64)));
    HIPCK(hipMemsetAsync(rk.scratch, 0, kScratchWords * sizeof(u64), rk.stream));
    TRY(ensure_csum(rk, 1024));
    HIPCK(hipStreamSynchronize(rk.stream));
    return MPX_OK;
}

// Frees what attach_resources allocated, on a failed attach: the stream is
// drained first and goes back to the pool (the teardown rule above
// create_rank_stream: free, never destroy).
void release_rank(Rank& rk) {
    if (rk.stream) (void)hipStreamSynchronize(rk.stream);
    free_rank_memory(rk);
    rk.ev0.reset();
    rk.ev1.reset();
    if (rk.stream) release_rank_stream(rk.dev, rk.stream);
    (void)hipGetLastError();
    rk = Rank{};
}

// Peer access between `dev` and the GPU of every local rank (ctx->mu held).
int enable_peer_access(mpx_ctx* ctx, int dev) {
    for (int i = 0; i < MPX_MAX_RANKS; ++i) {
        const Rank& o = ctx->r[i];
        if (!o.local || o.dev == dev) continue;
        int can = 0;
        HIPCK(hipDeviceCanAccessPeer(&can, dev, o.dev));
        if (!can) return fail(MPX_ERR_UNSUPPORTED, "GPU %d cannot access GPU %d (no xGMI/P2P path)", dev, o.dev);
        for (int dir = 0; dir < 2; ++dir) {
            const int a = dir ? o.dev : dev, b = dir ? dev : o.dev;
            DeviceGuard ga(a);
            const hipError_t e = hipDeviceEnablePeerAccess(b, 0);
            if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) HIPCK(e);
            (void)hipGetLastError();
        }
    }
    return MPX_OK;
}

}  // namespace

int mpx_rank_attach(mpx_ctx* ctx, int rank, int dev, void* tx, void* rx, size_t len) {
    if (!ctx) return fail(MPX_ERR_INVALID, "ctx is NULL");
    if (rank < 0 || rank >= ctx->nranks) return fail(MPX_ERR_INVALID, "rank %d not in [0,%d)", rank, ctx->nranks);
    if (!tx || !rx) return fail(MPX_ERR_INVALID, "NULL tx/rx");
    if (len > 0x7fffffffull) return fail(MPX_ERR_INVALID, "len %zu exceeds the reference's int buff_len", len);
    TRY(check_dev(dev));
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (ctx->r[rank].local || ctx->r[rank].imported || ctx->r[rank].host)
            return fail(MPX_ERR_STATE, "rank %d already registered", rank);
        auto it = ctx->allocs.find(reinterpret_cast<uintptr_t>(rx));
        if (it == ctx->allocs.end() || it->second.dev != dev || it->second.bytes < len)
            return fail(MPX_ERR_INVALID, "rx must be an mpx_alloc base on device %d of >= %zu bytes", dev, len);
        auto jt = ctx->allocs.find(reinterpret_cast<uintptr_t>(tx));
        if (jt == ctx->allocs.end() || jt->second.dev != dev || jt->second.bytes < len)
            return fail(MPX_ERR_INVALID, "tx must be an mpx_alloc base on device %d of >= %zu bytes", dev, len);
    }
    DeviceGuard g(dev);
    HIPCK(g.err);
    Rank rk;
    rk.local = true;
    rk.dev = dev;
    rk.tx = static_cast<unsigned char*>(tx);
    rk.rx = static_cast<unsigned char*>(rx);
    rk.len = len;
    int st = attach_resources(rk);
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (st == MPX_OK) st = enable_peer_access(ctx, dev);
    if (st != MPX_OK) {
        release_rank(rk);   // nothing of a failed attach stays allocated
        return st;
    }
    if (ctx->import_dev < 0) ctx->import_dev = dev;
    ctx->r[rank] = std::move(rk);
    return MPX_OK;
}

int mpx_rank_export(mpx_ctx* ctx, int rank, void* desc) {
    if (!ctx || !desc) return fail(MPX_ERR_INVALID, "NULL argument");
    if (rank < 0 || rank >= ctx->nranks || !ctx->r[rank].local) return fail(MPX_ERR_STATE, "rank %d is not a local rank", rank);
    const Rank& rk = ctx->r[rank];
    RankDesc d;
    memset(&d, 0, sizeof d);
    memcpy(d.magic, "MPXRANK2", 8);
    d.abi = MPX_ABI_VERSION;
    d.rank = rank;
    d.dev = rk.dev;
    d.mb_kind = rk.mb_kind;
    d.pid = (int64_t)getpid();
    d.len = rk.len;
    memcpy(d.bus_id, rk.bus_id, sizeof d.bus_id);
    gethostname(d.host, sizeof d.host - 1);
    DeviceGuard g(rk.dev);
    DBG("export rank %d: rx %p mb %p (kind %d) dev %d\n", rank, (void*)rk.rx, (void*)rk.mb, rk.mb_kind, rk.dev);
    HIPCK(hipIpcGetMemHandle(&d.rx_handle, rk.rx));
    HIPCK(hipIpcGetMemHandle(&d.tx_handle, rk.tx));
    HIPCK(hipIpcGetMemHandle(&d.mb_handle, rk.mb));
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        TRY(ensure_ring(ctx->r[rank]));
    }
    d.ring_bytes = rk.ring_bytes;
    if (rk.ring) HIPCK(hipIpcGetMemHandle(&d.ring_handle, rk.ring));
    memset(desc, 0, MPX_RANK_DESC_BYTES);
    memcpy(desc, &d, sizeof d);
    return MPX_OK;
}

int mpx_rank_import(mpx_ctx* ctx, int rank, const void* desc) {
    if (!ctx || !desc) return fail(MPX_ERR_INVALID, "NULL argument");
    if (rank < 0 || rank >= ctx->nranks) return fail(MPX_ERR_INVALID, "rank %d not in [0,%d)", rank, ctx->nranks);
    RankDesc d;
    memcpy(&d, desc, sizeof d);
    if (memcmp(d.magic, "MPXRANK2", 8) != 0 || d.abi != MPX_ABI_VERSION || d.rank != rank)
        return fail(MPX_ERR_INVALID, "descriptor is not an mpx rank %d descriptor", rank);
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (ctx->r[rank].local || ctx->r[rank].imported || ctx->r[rank].host)
        return fail(MPX_ERR_STATE, "rank %d already registered", rank);
    if (ctx->import_dev < 0) return fail(MPX_ERR_STATE, "attach a local rank before importing remote ranks");
    if (d.pid == (int64_t)getpid()) return fail(MPX_ERR_INVALID, "rank %d belongs to this process: attach it instead", rank);
    DeviceGuard g(ctx->import_dev);
    HIPCK(g.err);
    Rank rk;
    rk.imported = true;
    rk.dev = d.dev;
    memcpy(rk.bus_id, d.bus_id, sizeof rk.bus_id);
    rk.len = d.len;
    rk.mb_kind = d.mb_kind;
    void* p = nullptr;
    HIPCK(hipIpcOpenMemHandle(&p, d.mb_handle, hipIpcMemLazyEnablePeerAccess));
    ctx->ipc_opened.push_back(p);
    rk.mb = static_cast<Mailbox*>(p);
    HIPCK(hipIpcOpenMemHandle(&p, d.rx_handle, hipIpcMemLazyEnablePeerAccess));
    ctx->ipc_opened.push_back(p);
    rk.rx = static_cast<unsigned char*>(p);
    // tx is mapped on the first pull-mode call that loads from it
    // (ensure_peer_tx): a job that never pulls maps nothing more than before
    rk.tx_handle = d.tx_handle;
    rk.tx_handle_valid = true;
    rk.ring_bytes = d.ring_bytes;
    if (d.ring_bytes) {
        HIPCK(hipIpcOpenMemHandle(&p, d.ring_handle, hipIpcMemLazyEnablePeerAccess));
        ctx->ipc_opened.push_back(p);
        rk.ring = static_cast<unsigned char*>(p);
    }
    ctx->r[rank] = std::move(rk);
    return MPX_OK;
}

}  // extern "C"

namespace mpx {

// The state every transfer call needs of its rank and its peers (pair, armed
// and fan calls alike; my_rank and the peers are in range): the rank is
// attached in this process, every peer is known here, no earlier transfer of
// the rank timed out, and tx/rx are its attached buffers.
int check_rank_state(mpx_ctx* ctx, int my_rank, const void* tx, const void* rx, const int* peers, int npeers) {
    const Rank& me = ctx->r[my_rank];
    if (!me.local) return fail(MPX_ERR_STATE, "rank %d is not attached in this process", my_rank);
    for (int k = 0; k < npeers; ++k)
        if (!ctx->r[peers[k]].local && !ctx->r[peers[k]].imported)
            return fail(MPX_ERR_STATE, "peer rank %d is unknown (attach or import it)", peers[k]);
    if (me.broken) return fail(MPX_ERR_STATE, "rank %d: a previous transfer timed out", my_rank);
    if (tx != me.tx || rx != me.rx) return fail(MPX_ERR_INVALID, "tx/rx are not rank %d's attached buffers", my_rank);
    return MPX_OK;
}

// The mode / rank / iters / length checks of a transfer call (check_call) and
// of mpx_xfer_prepare, which passes no group: a prepare checks neither the
// group nor the self-pair rule.
int check_args(mpx_ctx* ctx, int mode, const int* my_group, int my_rank, int peer_rank, int iters, int buff_len) {
    if (mode < MPX_MODE_PINGPONG || mode > MPX_MODE_UNIDIR) return fail(MPX_ERR_INVALID, "mode %d", mode);
    if (my_group && *my_group != 0 && *my_group != 1) return fail(MPX_ERR_INVALID, "group %d", *my_group);
    if (my_rank < 0 || my_rank >= ctx->nranks || peer_rank < 0 || peer_rank >= ctx->nranks)
        return fail(MPX_ERR_INVALID, "ranks %d/%d", my_rank, peer_rank);
    // a rank paired with itself: only the symmetric non-blocking loop (Isend +
    // Irecv to itself, MPI's self-send) — the one-kernel loopback every engine
    // can run on one GPU (RCCL refuses two ranks on one device), and the form
    // a profiler that serialises dispatches can trace
    if (my_group && my_rank == peer_rank && mode != MPX_MODE_NONBLOCKING)
        return fail(MPX_ERR_INVALID, "rank %d paired with itself: only the non-blocking loop", my_rank);
    if (iters < 0 || buff_len < 0) return fail(MPX_ERR_INVALID, "iters %d, buff_len %d", iters, buff_len);
    return MPX_OK;
}

// Argument checks and per-rank set-up shared by mpx_xfer_ex and mpx_xfer_arm.
int check_call(mpx_ctx* ctx, int mode, int my_group, int my_rank, int peer_rank, int iters, void* tx, void* rx,
               int buff_len, const mpx_xfer_opts* opts) {
    TRY(check_args(ctx, mode, &my_group, my_rank, peer_rank, iters, buff_len));
    Rank& me = ctx->r[my_rank];
    Rank& peer = ctx->r[peer_rank];
    // RCCL addresses the peer by its communicator rank and maps nothing itself;
    // the kernel and SDMA engines write into the peer's rx and mailbox
    const bool rccl = ctx->engine == MPX_ENGINE_RCCL;
    TRY(check_rank_state(ctx, my_rank, tx, rx, &peer_rank, rccl ? 0 : 1));
    if ((size_t)buff_len > me.len || (!rccl && (size_t)buff_len > peer.len))
        return fail(MPX_ERR_INVALID, "buff_len %d exceeds an attached length (%zu, %zu)", buff_len, me.len, peer.len);
    const int check = opts && opts->check;
    if (opts && (opts->flags & MPX_XFER_PULL) && ctx->engine == MPX_ENGINE_RCCL)
        return fail(MPX_ERR_UNSUPPORTED, "pull mode (MPX_XFER_PULL): the kernel and SDMA engines only");
    const bool pull = ctx->engine != MPX_ENGINE_RCCL && pull_requested(opts);
    if (check) TRY(ensure_csum(me, iters));
    // (pull mode receives into rx in order: no receive ring)
    if (check && !pull && mode == MPX_MODE_NONBLOCKING && ctx->engine != MPX_ENGINE_RCCL) {
        // both ends of the link, under the lock: the other rank's thread may
        // be here too, and both must see both rings before sizing the slots
        std::lock_guard<std::mutex> lk(ctx->mu);
        TRY(ensure_ring(me));
        TRY(ensure_ring(peer));
    }
    return MPX_OK;
}

// The check-mode verdict of a completed call: reads `groups` x `per` checksum
// words of the rank back (group g: the receives of a pair call, or of link g
// of a fan call), finishes each with the length `n` and compares it with
// want[g].  bad[g] and digest[g] (either may be null) get the group's
// failures and the sum of its finished checksums; t gets the totals.  One
// device-to-host copy and one synchronise of the rank's own stream (a
// null-stream copy would wait for every blocking stream of the device, i.e.
// for other pairs' kernels) — which also drains whatever the caller enqueued
// on it before, with no group at all too.
// want_each (mpx_xfer_seq): an expectation per payload, want_each[g * per + i],
// in want[g]'s place.
int check_verdict(Rank& me, int my_rank, int groups, int per, u64 n, const uint64_t* want, mpx_timing* t, int* bad,
                  u64* digest, const uint64_t* want_each) {
    const size_t words = (size_t)groups * (size_t)per;
    std::vector<u64> raw(words);
    if (words) HIPCK(hipMemcpyAsync(raw.data(), me.csum, words * sizeof(u64), hipMemcpyDeviceToHost, me.stream));
    HIPCK(hipStreamSynchronize(me.stream));
    const u64 fmix = mix64_host(n);
    int total = 0;
    for (int g = 0; g < groups; ++g) {
        u64 sum = 0;
        int miss = 0;
        for (int i = 0; i < per; ++i) {
            const u64 c = raw[(size_t)g * per + i] ^ fmix;
            sum += c;
            if (c != (want_each ? want_each[(size_t)g * per + i] : want[g])) ++miss;
        }
        if (bad) bad[g] = miss;
        if (digest) digest[g] = sum;
        total += miss;
    }
    t->check_failures = total;
    t->check_iters = words;
    if (total)
        return fail(MPX_ERR_CHECK, "rank %d: %d of %zu received payloads failed the checksum", my_rank, total, words);
    return MPX_OK;
}

}  // namespace mpx

extern "C" {

namespace {
// After a completed loop: its algorithmic bytes and, in check mode, every
// received payload's checksum against the peer's tx — in the non-blocking
// loop too, where each receive has a slot of its own (k_xfer_nbcheck /
// SdmaNbChecked).
int finish_xfer(Rank& me, int mode, int my_group, int my_rank, int iters, int buff_len, const mpx_xfer_opts* opts,
                mpx_timing* t) {
    t->bytes = (uint64_t)buff_len * (uint64_t)iters * (mode == MPX_MODE_UNIDIR ? 1u : 2u);
    if (!(opts && opts->check) || iters <= 0) return MPX_OK;
    DeviceGuard g(me.dev);
    HIPCK(g.err);
    const bool ack = mode == MPX_MODE_UNIDIR && my_group == 1;
    const u64 n = ack ? 1 : (u64)buff_len;   // the ack is always 1 byte (mpi_perf.c:137,142)
    const uint64_t want = ack ? opts->expect_ack : opts->expect_checksum;
    return check_verdict(me, my_rank, 1, iters, n, &want, t, nullptr, nullptr);
}
}  // namespace

int mpx_xfer_ex(mpx_ctx* ctx, int mode, int my_group, int my_rank, int peer_rank, int iters, void* tx, void* rx,
                int buff_len, const mpx_xfer_opts* opts, mpx_timing* t) {
    if (!ctx || !t) return fail(MPX_ERR_INVALID, "NULL argument");
    memset(t, 0, sizeof *t);
    const double t_call = now_s();
    TRY(check_call(ctx, mode, my_group, my_rank, peer_rank, iters, tx, rx, buff_len, opts));
    Rank& me = ctx->r[my_rank];
    Rank& peer = ctx->r[peer_rank];
    const bool pull = ctx->engine != MPX_ENGINE_RCCL && pull_requested(opts);
    if (me.armed) {
        TRY(start_armed(me, my_rank, peer_rank, mode, my_group, iters, buff_len, opts, t_call, t));
        return finish_xfer(me, mode, my_group, my_rank, iters, buff_len, opts, t);
    }
    DeviceGuard g(me.dev);
    HIPCK(g.err);
    int st;
    switch (ctx->engine) {
        case MPX_ENGINE_KERNEL:
            st = run_kernel(ctx, me, peer, my_rank, peer_rank, mode, my_group, iters, buff_len, opts, t);
            break;
        case MPX_ENGINE_SDMA:
            st = pull && buff_len > 0 && !peer.tx ? ensure_peer_tx(ctx, peer, peer_rank) : MPX_OK;
            if (st == MPX_OK) st = run_sdma(me, peer, my_rank, peer_rank, mode, my_group, iters, buff_len, opts, t, pull);
            break;
        default: st = run_rccl(me, peer, my_rank, peer_rank, mode, my_group, iters, buff_len, opts, t); break;
    }
    if (st != MPX_OK) return st;
    return finish_xfer(me, mode, my_group, my_rank, iters, buff_len, opts, t);
}
int mpx_xfer(mpx_ctx* ctx, int mode, int my_group, int my_rank, int peer_rank, int iters, void* tx, void* rx,
             int buff_len, double* sec) {
    mpx_timing t;
    const int st = mpx_xfer_ex(ctx, mode, my_group, my_rank, peer_rank, iters, tx, rx, buff_len, nullptr, &t);
    if (sec) *sec = t.wall_s;
    return st;
}

// ---------------------------------------------------------------------------
// sequenced payloads (include/mpx_seq.h; k_xfer_seq, k_xfer_seq_nbcheck)
// ---------------------------------------------------------------------------
int mpx_seq_expect(uint64_t seed, int src, int dst, int iter, size_t n, uint64_t* out) {
    if (!out) return fail(MPX_ERR_INVALID, "NULL argument");
    if (src < 0 || src >= MPX_MAX_RANKS || dst < 0 || dst >= MPX_MAX_RANKS || iter < 0)
        return fail(MPX_ERR_INVALID, "ranks %d/%d, iteration %d", src, dst, iter);
    *out = seq::expect(seq::key_of(seq::key_base(seed, src, dst), iter), n);
    return MPX_OK;
}

int mpx_xfer_seq(mpx_ctx* ctx, int mode, int my_group, int my_rank, int peer_rank, int iters, void* tx, void* rx,
                 int buff_len, const mpx_seq_opts* opts, mpx_timing* t) {
    if (!ctx || !opts || !t) return fail(MPX_ERR_INVALID, "NULL argument");
    memset(t, 0, sizeof *t);
    // ---- refusals: all before any GPU work ------------------------------------
    if (ctx->engine != MPX_ENGINE_KERNEL) return fail(MPX_ERR_UNSUPPORTED, "mpx_xfer_seq: the kernel engine only");
    if (pull_requested(nullptr))
        return fail(MPX_ERR_UNSUPPORTED,
                    "mpx_xfer_seq with MPX_XFER_PULL set: a pulled payload would have to be written into tx first");
    if (opts->flags & ~MPX_XFER_STREAM)
        return fail(MPX_ERR_INVALID, "flags %#x: only MPX_XFER_STREAM (a sequenced call reads no tx to stage or pull)",
                    opts->flags);
    TRY(check_args(ctx, mode, &my_group, my_rank, peer_rank, iters, buff_len));
    const bool ack = mode == MPX_MODE_UNIDIR && my_group == 1;
    const u64 recv_len = ack ? 1 : (u64)buff_len;   // the ack is always 1 byte (mpi_perf.c:137,142)
    const bool check = opts->check != 0;
    if (check && !opts->expect && (u64)iters * recv_len > MPX_SEQ_AUTO_MAX)
        return fail(MPX_ERR_INVALID, "expect == NULL with %d x %llu B to generate on the CPU: above MPX_SEQ_AUTO_MAX (%llu)",
                    iters, recv_len, (u64)MPX_SEQ_AUTO_MAX);
    // a rank's state before its buffers' set-up (check_call: the checksum words and the check ring)
    if (my_rank >= 0 && my_rank < ctx->nranks && ctx->r[my_rank].armed)
        return fail(MPX_ERR_STATE, "rank %d holds an armed call (a sequenced call cannot be armed: start or disarm it first)",
                    my_rank);
    mpx_xfer_opts o{};
    o.check = check ? 1 : 0;
    o.flags = opts->flags;
    o.timeout_ms = opts->timeout_ms;
    o.nwg = opts->nwg;
    TRY(check_call(ctx, mode, my_group, my_rank, peer_rank, iters, tx, rx, buff_len, &o));
    Rank& me = ctx->r[my_rank];
    Rank& peer = ctx->r[peer_rank];
    const u64 keys[2] = {seq::key_base(opts->seed, my_rank, peer_rank), seq::key_base(opts->seed, peer_rank, my_rank)};
    // the expectations the caller left to the library: on the CPU, before the timed call
    std::vector<uint64_t> own;
    const uint64_t* want = opts->expect;
    if (check && !want) {
        own.resize((size_t)iters);
        for (int i = 0; i < iters; ++i) own[(size_t)i] = seq::expect(seq::key_of(keys[1], i), (size_t)recv_len);
        want = own.data();
    }
    DeviceGuard g(me.dev);
    HIPCK(g.err);
    TRY(run_kernel(ctx, me, peer, my_rank, peer_rank, mode, my_group, iters, buff_len, &o, t, keys));
    t->bytes = (uint64_t)buff_len * (uint64_t)iters * (mode == MPX_MODE_UNIDIR ? 1u : 2u);
    if (!check || iters <= 0) return MPX_OK;
    return check_verdict(me, my_rank, 1, iters, recv_len, nullptr, t, nullptr, nullptr, want);
}

int mpx_shutdown(void) {
    StreamPool& p = pool();
    std::lock_guard<std::mutex> lk(p.mu);
    if (p.live_contexts != 0) return fail(MPX_ERR_STATE, "%d contexts are still alive", p.live_contexts);
    if (p.all.empty()) return MPX_OK;
    if (!callback_fence(p.all))
        return fail(MPX_ERR_TIMEOUT, "stream fence did not complete in 10 s: streams left to the runtime");
    // every stream is destroyed and forgotten, whatever one destroy returns
    // (a stream left in the pool after a failed destroy could be handed out
    // again, or destroyed twice by a second shutdown); the first error is
    // the result, reported after the caller's device is restored
    int prev = -1;
    (void)hipGetDevice(&prev);
    hipError_t first = hipSuccess;
    int first_dev = -1;
    for (auto& ds : p.all) {
        (void)hipSetDevice(ds.first);
        const hipError_t e = hipStreamDestroy(ds.second);
        if (e != hipSuccess && first == hipSuccess) {
            first = e;
            first_dev = ds.first;
        }
    }
    (void)hipGetLastError();
    if (prev >= 0) (void)hipSetDevice(prev);
    p.all.clear();
    p.idle.clear();
    if (first != hipSuccess)
        return fail(MPX_ERR_HIP, "hipStreamDestroy on device %d: %s", first_dev, hipGetErrorString(first));
    return MPX_OK;
}

int mpx_live_events(int* count) {
    if (!count) return fail(MPX_ERR_INVALID, "NULL argument");
    *count = live_events().load();
    return MPX_OK;
}

int mpx_link_counters(mpx_ctx* ctx, int my_rank, int peer_rank, uint64_t out[4]) {
    if (!ctx || !out) return fail(MPX_ERR_INVALID, "NULL argument");
    // (either end of a host link: a host endpoint counts its links as a local rank does)
    if (my_rank < 0 || my_rank >= ctx->nranks || !(ctx->r[my_rank].local || ctx->r[my_rank].host))
        return fail(MPX_ERR_INVALID, "rank %d is not a local rank", my_rank);
    if (peer_rank < 0 || peer_rank >= ctx->nranks) return fail(MPX_ERR_INVALID, "peer rank %d", peer_rank);
    const Rank& me = ctx->r[my_rank];
    out[0] = me.tx_seq[peer_rank];
    out[1] = me.rx_seq[peer_rank];
    out[2] = me.calls[peer_rank];
    out[3] = me.host ? 0 : me.token;
    return MPX_OK;
}

// Test-only (the MPX_TEST gate of test_knobs): the link's counters jump
// forward, as a long run would have left them.  Every mailbox compare is
// "word >= a value derived from these counters" and the mailbox holds only
// values of the link's past, so a forward jump made alike on both ranks of the
// link is a state the link can reach (the one exception: the LL
// zone's 2^31 alias).
int mpx_test_advance_link(mpx_ctx* ctx, int my_rank, int peer_rank, uint64_t seq_by, uint64_t calls_by,
                          uint64_t token_by) {
    if (!ctx) return fail(MPX_ERR_INVALID, "NULL argument");
    if (!test_gate()) return fail(MPX_ERR_UNSUPPORTED, "mpx_test_advance_link: the process started without MPX_TEST");
    // (either end of a host link, as mpx_link_counters: a host endpoint has no token to move)
    if (my_rank < 0 || my_rank >= ctx->nranks || !(ctx->r[my_rank].local || ctx->r[my_rank].host))
        return fail(MPX_ERR_INVALID, "rank %d is not a local rank", my_rank);
    if (peer_rank < 0 || peer_rank >= ctx->nranks) return fail(MPX_ERR_INVALID, "peer rank %d", peer_rank);
    Rank& me = ctx->r[my_rank];
    if (me.host && token_by) return fail(MPX_ERR_INVALID, "host endpoint %d has no token (token_by must be 0)", my_rank);
    if (me.armed) return fail(MPX_ERR_STATE, "rank %d holds an armed call (start or disarm it first)", my_rank);
    if (me.broken) return fail(MPX_ERR_STATE, "rank %d: a previous transfer timed out", my_rank);
    const u64 top = ~0ull;
    if (seq_by > top - me.tx_seq[peer_rank] || seq_by > top - me.rx_seq[peer_rank] ||
        calls_by > top - me.calls[peer_rank] || token_by > top - me.token)
        return fail(MPX_ERR_INVALID, "rank %d: a counter would pass 2^64", my_rank);
    me.tx_seq[peer_rank] += seq_by;
    me.rx_seq[peer_rank] += seq_by;
    me.calls[peer_rank] += calls_by;
    me.token += token_by;
    return MPX_OK;
}

int mpx_last_phases(mpx_ctx* ctx, int rank, mpx_phases* out) {
    if (!ctx || !out) return fail(MPX_ERR_INVALID, "NULL argument");
    if (rank < 0 || rank >= ctx->nranks || !ctx->r[rank].local) return fail(MPX_ERR_STATE, "rank %d is not a local rank", rank);
    *out = ctx->r[rank].phases;
    return MPX_OK;
}

// ---- latency recorders (include/mpx.h, include/mpx_fan_lat.h) ---------------
// mpx_lat_*: one block per rank, written by the blocking pair loops.
// mpx_fan_lat_*: ctx->nranks blocks per rank, keyed by peer rank, written by
// the LL fan exchange's links.  One set of helpers over Recorder; every entry
// point keeps its own argument checks, status codes and messages.
namespace {
// The rank a recorder call names: local (else `not_local`), and holding no
// armed call — an armed kernel is already running on the rank's stream, which
// every recorder call uses (and has read its recorder pointer).
int rec_rank(mpx_ctx* ctx, int rank, int not_local, Rank** out) {
    if (!ctx) return fail(MPX_ERR_INVALID, "ctx is NULL");
    if (rank < 0 || rank >= ctx->nranks || !ctx->r[rank].local) return fail(not_local, "rank %d is not a local rank", rank);
    if (ctx->r[rank].armed) return fail(MPX_ERR_STATE, "rank %d holds an armed call (start or disarm it first)", rank);
    *out = &ctx->r[rank];
    return MPX_OK;
}
int lat_rank(mpx_ctx* ctx, int rank, Rank** out) { return rec_rank(ctx, rank, MPX_ERR_STATE, out); }
int fan_lat_rank(mpx_ctx* ctx, int rank, Rank** out) { return rec_rank(ctx, rank, MPX_ERR_INVALID, out); }
int fan_lat_peer(const mpx_ctx* ctx, int rank, int peer) {
    if (peer < 0 || peer >= ctx->nranks || peer == rank) return fail(MPX_ERR_INVALID, "rank %d: peer rank %d", rank, peer);
    return MPX_OK;
}
// Every block: statistics, histogram and raw count back to zero, raw_cap in
// force; on the rank's stream, so the rank's next kernel starts behind it.
int rec_clear(Rank& me, const Recorder& rc) {
    LatBlock h{};
    h.raw_cap = (u64)rc.cap;
    for (int i = 0; i < rc.blocks; ++i)
        HIPCK(hipMemcpyAsync(rc.block(i), &h, offsetof(LatBlock, raw), hipMemcpyHostToDevice, me.stream));
    HIPCK(hipStreamSynchronize(me.stream));
    return MPX_OK;
}
int rec_header(Rank& me, const Recorder& rc, int i, LatBlock* h) {
    // the rank's own stream: behind the rank's last kernel (an armed call's
    // completion word comes before its kernel retires), and no wait for
    // other ranks' kernels (finish_xfer)
    HIPCK(hipMemcpyAsync(h, rc.block(i), offsetof(LatBlock, raw), hipMemcpyDeviceToHost, me.stream));
    HIPCK(hipStreamSynchronize(me.stream));
    return MPX_OK;
}
// Allocates (or regrows, for a larger raw_cap) `blocks` blocks, puts raw_cap in
// force, clears them and turns the recorder on.  A smaller raw_cap keeps the
// allocation: `blocks` blocks at the smaller stride fit it.
int rec_enable(Rank& me, Recorder& rc, int blocks, int raw_cap, int cap_max, const char* what) {
    if (raw_cap < 0 || raw_cap > cap_max) return fail(MPX_ERR_INVALID, "raw_cap %d not in [0,%d]", raw_cap, cap_max);
    DeviceGuard g(me.dev);
    HIPCK(g.err);
    if (!rc.base || rc.alloc < raw_cap) {
        // (no hipFree here: it waits for the whole device, ensure_csum)
        const size_t bytes = (size_t)blocks * lat_block_bytes(raw_cap);
        void* p = nullptr;
        const hipError_t e = hipMalloc(&p, bytes);
        if (e == hipErrorOutOfMemory) {
            (void)hipGetLastError();
            return fail(MPX_ERR_NOMEM, "%s of %zu B on device %d", what, bytes, me.dev);
        }
        HIPCK(e);
        if (rc.base) me.retired.push_back(rc.base);
        rc.base = static_cast<unsigned char*>(p);
        rc.blocks = blocks;
        rc.alloc = raw_cap;
    }
    rc.cap = raw_cap;
    rc.on = false;
    TRY(rec_clear(me, rc));
    rc.on = true;
    return MPX_OK;
}
int rec_reset(Rank& me, const Recorder& rc) {
    DeviceGuard g(me.dev);
    HIPCK(g.err);
    return rec_clear(me, rc);
}
int rec_get(Rank& me, const Recorder& rc, int i, mpx_lat* out) {
    DeviceGuard g(me.dev);
    HIPCK(g.err);
    LatBlock h{};
    TRY(rec_header(me, rc, i, &h));
    memset(out, 0, sizeof *out);
    out->count = h.count;
    out->calls = h.calls;
    out->min_ticks = h.min_ticks;
    out->max_ticks = h.max_ticks;
    out->sum_ticks = h.sum_ticks;
    out->max_iter = h.max_iter;
    out->last_iters = h.last_iters;
    out->tick_s = 1e-8;   // s_memrealtime: 100 MHz
    static_assert(sizeof out->hist == sizeof h.hist, "mpx_lat and LatBlock histograms differ");
    memcpy(out->hist, h.hist, sizeof h.hist);
    return MPX_OK;
}
// The last traced call's stamps of block i: at most cap, raw_cap + 1 and raw_n.
int rec_raw(Rank& me, const Recorder& rc, int i, uint64_t* stamps, int cap, int* n) {
    DeviceGuard g(me.dev);
    HIPCK(g.err);
    LatBlock h{};
    TRY(rec_header(me, rc, i, &h));
    // t[0] alone says nothing: with raw_cap = 0 no stamp is reported
    u64 have = rc.cap > 0 ? h.raw_n : 0;
    if (have > (u64)rc.cap + 1) have = (u64)rc.cap + 1;
    if (have > (u64)cap) have = (u64)cap;
    if (have) {
        HIPCK(hipMemcpyAsync(stamps, rc.block(i)->raw, (size_t)have * sizeof(u64), hipMemcpyDeviceToHost, me.stream));
        HIPCK(hipStreamSynchronize(me.stream));
    }
    *n = (int)have;
    return MPX_OK;
}
}  // namespace

int mpx_lat_enable(mpx_ctx* ctx, int rank, int raw_cap) {
    if (!ctx) return fail(MPX_ERR_INVALID, "ctx is NULL");
    if (ctx->engine != MPX_ENGINE_KERNEL)
        return fail(MPX_ERR_UNSUPPORTED, "the latency recorder runs inside the kernel engine's loop: not this engine");
    Rank* me = nullptr;
    TRY(lat_rank(ctx, rank, &me));
    return rec_enable(*me, me->lat, 1, raw_cap, MPX_LAT_RAW_MAX, "latency recorder");
}

int mpx_lat_disable(mpx_ctx* ctx, int rank) {
    Rank* me = nullptr;
    TRY(lat_rank(ctx, rank, &me));
    me->lat.on = false;   // the block stays until finalize (no hipFree between calls)
    return MPX_OK;
}

int mpx_lat_reset(mpx_ctx* ctx, int rank) {
    Rank* me = nullptr;
    TRY(lat_rank(ctx, rank, &me));
    if (!me->lat.on) return fail(MPX_ERR_STATE, "rank %d: the latency recorder is not enabled", rank);
    return rec_reset(*me, me->lat);
}

int mpx_lat_get(mpx_ctx* ctx, int rank, mpx_lat* out) {
    Rank* me = nullptr;
    TRY(lat_rank(ctx, rank, &me));
    if (!out) return fail(MPX_ERR_INVALID, "NULL argument");
    if (!me->lat.on) return fail(MPX_ERR_STATE, "rank %d: the latency recorder is not enabled", rank);
    return rec_get(*me, me->lat, 0, out);
}

int mpx_lat_raw(mpx_ctx* ctx, int rank, uint64_t* stamps, int cap, int* n) {
    Rank* me = nullptr;
    TRY(lat_rank(ctx, rank, &me));
    if (!n || cap < 0 || (!stamps && cap > 0)) return fail(MPX_ERR_INVALID, "bad argument");
    *n = 0;
    if (!me->lat.on) return fail(MPX_ERR_STATE, "rank %d: the latency recorder is not enabled", rank);
    return rec_raw(*me, me->lat, 0, stamps, cap, n);
}

int mpx_fan_lat_enable(mpx_ctx* ctx, int rank, int raw_cap) {
    if (!ctx) return fail(MPX_ERR_INVALID, "ctx is NULL");
    if (ctx->engine != MPX_ENGINE_KERNEL)
        return fail(MPX_ERR_UNSUPPORTED, "the link recorder runs inside the kernel engine's LL fan loop: not this engine");
    Rank* me = nullptr;
    TRY(fan_lat_rank(ctx, rank, &me));
    return rec_enable(*me, me->fan_lat, ctx->nranks, raw_cap, MPX_FAN_LAT_RAW_MAX, "link recorder");
}

int mpx_fan_lat_disable(mpx_ctx* ctx, int rank) {
    Rank* me = nullptr;
    TRY(fan_lat_rank(ctx, rank, &me));
    me->fan_lat.on = false;   // the blocks stay until finalize (no hipFree between calls)
    return MPX_OK;
}

int mpx_fan_lat_reset(mpx_ctx* ctx, int rank) {
    Rank* me = nullptr;
    TRY(fan_lat_rank(ctx, rank, &me));
    if (!me->fan_lat.on) return fail(MPX_ERR_STATE, "rank %d: the link recorder is not enabled", rank);
    return rec_reset(*me, me->fan_lat);
}

int mpx_fan_lat_get(mpx_ctx* ctx, int rank, int peer, mpx_lat* out) {
    Rank* me = nullptr;
    TRY(fan_lat_rank(ctx, rank, &me));
    if (!out) return fail(MPX_ERR_INVALID, "NULL argument");
    TRY(fan_lat_peer(ctx, rank, peer));
    if (!me->fan_lat.on) return fail(MPX_ERR_STATE, "rank %d: the link recorder is not enabled", rank);
    return rec_get(*me, me->fan_lat, peer, out);
}

int mpx_fan_lat_raw(mpx_ctx* ctx, int rank, int peer, uint64_t* stamps, int cap, int* n) {
    Rank* me = nullptr;
    TRY(fan_lat_rank(ctx, rank, &me));
    if (!n || cap < 0 || (!stamps && cap > 0)) return fail(MPX_ERR_INVALID, "bad argument");
    *n = 0;
    TRY(fan_lat_peer(ctx, rank, peer));
    if (!me->fan_lat.on) return fail(MPX_ERR_STATE, "rank %d: the link recorder is not enabled", rank);
    return rec_raw(*me, me->fan_lat, peer, stamps, cap, n);
}

}  // extern "C"

// the Recorder helpers for the host-link recorder's GPU end (mpx_engine_hostlink.hip)
namespace mpx {
int recorder_enable(Rank& me, Recorder& rc, int blocks, int raw_cap, int cap_max, const char* what) {
    return rec_enable(me, rc, blocks, raw_cap, cap_max, what);
}
int recorder_reset(Rank& me, const Recorder& rc) { return rec_reset(me, rc); }
int recorder_get(Rank& me, const Recorder& rc, int i, mpx_lat* out) { return rec_get(me, rc, i, out); }
int recorder_raw(Rank& me, const Recorder& rc, int i, uint64_t* stamps, int cap, int* n) {
    return rec_raw(me, rc, i, stamps, cap, n);
}
}  // namespace mpx

extern "C" {

int mpx_barrier(mpx_ctx* ctx, int nthreads) {
    if (!ctx || nthreads < 1) return fail(MPX_ERR_INVALID, "bad argument");
    std::unique_lock<std::mutex> lk(ctx->bmu);
    const u64 gen = ctx->bgen;
    if (++ctx->bcount == nthreads) {
        ctx->bcount = 0;
        ++ctx->bgen;
        ctx->bcv.notify_all();
    } else {
        ctx->bcv.wait(lk, [&] { return ctx->bgen != gen; });
    }
    return MPX_OK;
}
}  // extern "C"
