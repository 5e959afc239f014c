// mpx_runtime.h — what the parts of libmpx's host side share: error
// reporting, the RAII holders, Rank and mpx_ctx, and the helpers more than one
// part calls.  The parts: mpx_runtime.hip (contexts, buffers, registration,
// copy, latency recorder, the C-ABI), mpx_engine_kernel.hip (the kernel
// engine's call lifecycle: pair, armed, fan and host-link calls),
// mpx_engine_hostlink.hip (host endpoints and both sides of a host-link call)
// and mpx_engine_stream.hip (the SDMA and RCCL engines).  Nothing here is
// exported from libmpx.so.
#pragma once

#include "mpx_internal.h"

#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>
#include <rccl/rccl.h>   // types only: the functions are bound at run time (rccl_api)

#include <atomic>
#include <condition_variable>
#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <type_traits>
#include <vector>

#include <dlfcn.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <time.h>
#include <unistd.h>

#pragma GCC visibility push(hidden)

namespace mpx {

// Sets the thread's last error (mpx_last_error) and returns `code`.
int fail(int code, const char* fmt, ...);

#define HIPCK(expr)                                                                                 \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess)                                                                       \
            return fail(MPX_ERR_HIP, "%s:%d %s: %s", __FILE__, __LINE__, #expr, hipGetErrorString(e_)); \
    } while (0)

// RCCL's entry points, bound at run time (rccl_api, mpx_engine_stream.hip).
struct RcclApi {
    void* h = nullptr;
    char path[512] = {0};
    char error[512] = {0};
    ncclResult_t (*GetVersion)(int*) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
};
const RcclApi& rccl_api();

inline double now_s() {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec + ts.tv_nsec * 1e-9;
}

inline u64 mix64_host(u64 z) {
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// Restores the calling thread's current device on scope exit.
struct DeviceGuard {
    int prev = -1;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        err = hipSetDevice(dev);
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// Owns one HIP event: destroyed when its holder goes (scope exit on any
// path, an early HIPCK return included, or the owning Rank's reset), so no
// error path can leak it.  live_events() counts the events alive in the
// process (mpx_live_events: the tests' leak check).
std::atomic<int>& live_events();

class Event {
  public:
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    Event(Event&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }
    Event& operator=(Event&& o) noexcept {
        if (this != &o) {
            reset();
            e_ = o.e_;
            o.e_ = nullptr;
        }
        return *this;
    }
    ~Event() { reset(); }
    hipError_t create() {
        reset();
        const hipError_t e = hipEventCreate(&e_);
        if (e == hipSuccess) live_events().fetch_add(1);
        else e_ = nullptr;
        return e;
    }
    void reset() {
        if (!e_) return;
        (void)hipEventDestroy(e_);
        e_ = nullptr;
        live_events().fetch_sub(1);
    }
    operator hipEvent_t() const { return e_; }

  private:
    hipEvent_t e_ = nullptr;
};

enum MailboxKind { kMbUncached = 0, kMbFine = 1, kMbCoarse = 2 };

// (mode, group, peer rank, bytes, timeout ticks, iterations) of a captured
// SDMA chunk
typedef std::tuple<int, int, int, long long, u64, int> SdmaKey;

// A latency recorder's device memory (mpx_lat_*, mpx_fan_lat_*): `blocks`
// LatBlocks, stride() apart.  The allocation holds `blocks` blocks of raw_cap
// `alloc`; cap <= alloc is the raw_cap in force, so the blocks at its stride
// fit the allocation.
struct Recorder {
    unsigned char* base = nullptr;
    int blocks = 0;
    int alloc = 0;                 // raw_cap the blocks were allocated for
    int cap = 0;                   // raw_cap in force (the blocks' stride)
    bool on = false;               // the rank's calls are traced
    size_t stride() const { return lat_block_bytes(cap); }
    LatBlock* block(int i) const { return reinterpret_cast<LatBlock*>(base + (size_t)i * stride()); }
};

struct Rank {
    bool local = false;
    bool imported = false;
    bool broken = false;           // a transfer timed out: link state unknown
    // a host endpoint (mpx_host_attach): neither local nor imported.  tx, rx and
    // len are its pinned host buffers (CPU pointers); tx_seq / rx_seq / calls
    // count as a local rank's and are touched only by mpx_host_xfer's thread
    bool host = false;
    void* host_mb = nullptr;       // its hostlink::HostMailbox, as the CPU addresses it
    unsigned char* host_tx_dev = nullptr;   // tx, rx and the mailbox as the GPUs address them
    unsigned char* host_rx_dev = nullptr;
    void* host_mb_dev = nullptr;
    int dev = -1;
    char bus_id[32] = {0};
    unsigned char* tx = nullptr;   // local tx, or the imported rank's tx mapped here (pull mode:
                                   // on the first pull call, ensure_peer_tx)
    hipIpcMemHandle_t tx_handle{}; // imported rank: its tx, until mapped
    bool tx_handle_valid = false;
    unsigned char* rx = nullptr;   // local rx, or the imported rank's rx mapped here
    size_t len = 0;
    Mailbox* mb = nullptr;         // usable from this process
    int mb_kind = kMbUncached;
    hipStream_t stream = nullptr;
    Event ev0, ev1;                // start / end of the rank's last call (RAII)
    u64 token = 0;                 // kernel-engine calls made: Status.done of the last one
    mpx_phases phases{};           // the last kernel-engine call (mpx_last_phases)
    struct KernelCall* armed = nullptr;   // the call mpx_xfer_arm launched, not started yet
    Status* status = nullptr;      // host-mapped (local ranks)
    u64* scratch = nullptr;        // kScratchWords device words (local ranks)
    u64* csum = nullptr;           // per-iteration checksums (device), csum_cap words,
    u64* cnt = nullptr;            //   then cnt: checked chunks per receive (csum + csum_cap)
    size_t csum_cap = 0;
    unsigned char* ring = nullptr; // non-blocking check mode's receive slots 1..S-1
    uint64_t ring_bytes = 0;       //   (allocated on first use, or at export: ensure_ring)
    std::vector<void*> retired;    // outgrown csum arrays and recorder blocks (freed at finalize)
    Recorder lat;                  // latency recorder (mpx_lat_enable): one block; on: blocking calls are traced
    Recorder fan_lat;              // link recorder (mpx_fan_lat_enable): ctx->nranks blocks, keyed by peer
                                   //   rank; on: MPX_FAN_LL calls of this rank are traced per link
    Recorder hostlink_lat;         // host-link recorder (mpx_hostlink_lat_enable): ctx->nranks blocks, keyed by
                                   //   the endpoint's rank; on: this rank's mpx_xfer_hostlink calls are traced
    // a host endpoint's host-link recorder: ctx->nranks hostlink::LatRec blocks in
    // ordinary host memory (malloc), keyed by the GPU peer's rank, host_lat_stride
    // apart; touched only by mpx_host_xfer's thread and, between its calls, the caller
    unsigned char* host_lat = nullptr;
    int host_lat_alloc = 0;        //   raw_cap the blocks were allocated for
    int host_lat_cap = 0;          //   raw_cap in force (the blocks' stride)
    bool host_lat_on = false;
    FanTable* fan_tab = nullptr;   // fan exchange (mpx_xfer_fan): the link table in device memory
    FanTable* fan_host = nullptr;  //   and its pinned host image (allocated on the first fan call)
    u64 tx_seq[MPX_MAX_RANKS] = {};
    u64 rx_seq[MPX_MAX_RANKS] = {};
    u64 calls[MPX_MAX_RANKS] = {};   // transfer calls on the link to that rank (Mailbox.posted)
    ncclComm_t comm = nullptr;
    int comm_rank = -1;
    bool rccl_linked[MPX_MAX_RANKS] = {};          // RCCL p2p channel to that rank set up (mpx_xfer_prepare)
    std::map<SdmaKey, hipGraphExec_t> sdma_graphs;   // run_sdma's captured chunks
};

struct AllocRec {
    int dev;
    size_t bytes;
};

}  // namespace mpx

#pragma GCC visibility pop
struct mpx_ctx {   // (the opaque type of include/mpx.h: declared there with default visibility)
    int nranks = 0;
    int engine = 0;
    std::mutex mu;
    mpx::Rank r[MPX_MAX_RANKS];
    std::map<uintptr_t, mpx::AllocRec> allocs;
    std::map<int, hipStream_t> dev_stream;     // utility stream per device
    std::map<int, u64*> dev_tmp;               // 8-byte device scratch per device
    std::vector<void*> ipc_opened;             // to close on finalize
    std::mutex util_mu;                        // fill / checksum / copy share dev_stream + dev_tmp
    int import_dev = -1;
    // barrier (mpx_barrier)
    std::mutex bmu;
    std::condition_variable bcv;
    int bcount = 0;
    u64 bgen = 0;
};
#pragma GCC visibility push(hidden)

namespace mpx {

// receive slots of the link between two ranks: the same on both sides
inline int link_slots(const Rank& a, const Rank& b, long long len) {
    const int sa = ring_slots(a.ring_bytes, len), sb = ring_slots(b.ring_bytes, len);
    return sa < sb ? sa : sb;
}

inline bool same_device(const Rank& a, const Rank& b) {
    if (a.local && b.local) return a.dev == b.dev;
    return a.bus_id[0] && strcmp(a.bus_id, b.bus_id) == 0;
}

inline u64 timeout_ticks_ms(uint32_t timeout_ms) {
    const u64 ms = timeout_ms ? timeout_ms : 10000;
    return ms * 100000ull;   // s_memrealtime runs at 100 MHz
}
inline u64 timeout_ticks(const mpx_xfer_opts* o) { return timeout_ticks_ms(o ? o->timeout_ms : 0); }

// The tests' fault injection (MPX_TEST; the knobs are described at
// test_knobs, mpx_runtime.hip).
struct TestKnobs {
    int skip_push = 0;
    int lag_rank = -1, lag_wg = 0;
    long long lag_us = 0;
    bool no_posted = false, no_pull_wait = false;
    int host_lag_iter = -1;        // host_lag=<iter>:<us>: a host endpoint stalls before that iteration
    long long host_lag_us = 0;
    int seq_stale = 0;             // seq_stale=<k>: an endpoint's k-th sequenced send repeats the payload before it
    int fail_launch = -1;
    bool fail_copy = false;
};
TestKnobs test_knobs();

// ---- mpx_runtime.hip -------------------------------------------------------
int ensure_csum(Rank& rk, int iters);
int nb_publish();
bool pull_requested(const mpx_xfer_opts* o);
// a Recorder's life (mpx_lat_*, mpx_fan_lat_*; mpx_engine_hostlink.hip: mpx_hostlink_lat_* on a GPU rank)
int recorder_enable(Rank& me, Recorder& rc, int blocks, int raw_cap, int cap_max, const char* what);
int recorder_reset(Rank& me, const Recorder& rc);
int recorder_get(Rank& me, const Recorder& rc, int i, mpx_lat* out);
int recorder_raw(Rank& me, const Recorder& rc, int i, uint64_t* stamps, int cap, int* n);
int ensure_peer_tx(mpx_ctx* ctx, Rank& peer, int peer_rank);
int ensure_peer_tx_locked(mpx_ctx* ctx, Rank& peer, int peer_rank);
int check_rank_state(mpx_ctx* ctx, int my_rank, const void* tx, const void* rx, const int* peers, int npeers);
int check_args(mpx_ctx* ctx, int mode, const int* my_group, int my_rank, int peer_rank, int iters, int buff_len);
int check_call(mpx_ctx* ctx, int mode, int my_group, int my_rank, int peer_rank, int iters, void* tx, void* rx,
               int buff_len, const mpx_xfer_opts* opts);
int check_verdict(Rank& me, int my_rank, int groups, int per, u64 n, const uint64_t* want, mpx_timing* t, int* bad,
                  u64* digest, const uint64_t* want_each = nullptr);

// ---- mpx_engine_kernel.hip: the kernel engine --------------------------------
// seq_keys (mpx_xfer_seq): {send base, receive base} of a sequenced call, which
// runs the k_xfer_seq kernels; null: an ordinary call
int run_kernel(mpx_ctx* ctx, Rank& me, Rank& peer, int my_rank, int peer_rank, int mode, int group, int iters,
               long long len, const mpx_xfer_opts* o, mpx_timing* t, const u64* seq_keys = nullptr);
int start_armed(Rank& me, int my_rank, int peer_rank, int mode, int group, int iters, long long len,
                const mpx_xfer_opts* o, double t_call, mpx_timing* t);
int disarm(Rank& me);
// a host-link call's kernel through the one call lifecycle: takes the call's
// numbers on the link to host_rank (a.call, a.done_token), launches
// k_xfer_hostlink and completes the call as a pair call's
int run_hostlink_kernel(Rank& me, int my_rank, int host_rank, XferArgs& a, int grid, bool ll, double t_call,
                        mpx_timing* t);
// the same with k_hostlink_duplex (mpx_xfer_hostlink_duplex): a grid of 2 * a.nwg
int run_hostlink_duplex_kernel(Rank& me, int my_rank, int host_rank, XferArgs& a, double t_call, mpx_timing* t);

// ---- mpx_engine_hostlink.hip: the host link ----------------------------------
void free_host_endpoint(Rank& rk);   // mpx_finalize: a host endpoint's pinned memory

// ---- mpx_engine_stream.hip: the SDMA and RCCL engines ------------------------
int run_sdma(Rank& me, Rank& peer, int my_rank, int peer_rank, int mode, int group, int iters, long long len,
             const mpx_xfer_opts* o, mpx_timing* t, bool pull);
int run_rccl(Rank& me, Rank& peer, int my_rank, int peer_rank, int mode, int group, int iters, long long len,
             const mpx_xfer_opts* o, mpx_timing* t);

}  // namespace mpx

#pragma GCC visibility pop
