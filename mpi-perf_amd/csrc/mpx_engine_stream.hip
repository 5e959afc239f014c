// mpx_engine_stream.hip — the two stream engines behind mpx_xfer_ex: SDMA
// (run_sdma) and RCCL (run_rccl, with its run-time loader and the mpx_rccl_*
// entry points), and what prepares them ahead of a call (mpx_xfer_prepare).
// Both enqueue ONE loop, mpx_stream_loop.h's, on the rank's stream between one
// begin (stream_begin) and one end (stream_end); what an iteration enqueues is
// in four operations objects: SdmaPush, SdmaPull, SdmaNbChecked and RcclOps
// (DESIGN.md "Stream engines").
#include "mpx_runtime.h"
#include "mpx_stream_loop.h"

using namespace mpx;

namespace mpx {

// RCCL is bound at run time from ONE file, the image's /opt/rocm/lib/librccl.so.1
// (MPX_RCCL_LIB overrides), opened RTLD_LOCAL | RTLD_DEEPBIND: no symbol of it
// enters the process's global scope, and its own references resolve inside
// it.  A process that already holds another librccl.so.1 (torch's bundled
// 2.26.6 in bench.py) therefore cannot shadow it, and bench.py and mpx_perf
// run the same RCCL.  Linking -lrccl bound libmpx to
// whichever librccl.so.1 the process had loaded first.
const RcclApi& rccl_api() {
    static const RcclApi* api = [] {
        RcclApi* a = new RcclApi;   // never destroyed, never dlclosed (exit-time ordering)
        const char* want = getenv("MPX_RCCL_LIB");
        if (!want || !*want) want = "/opt/rocm/lib/librccl.so.1";
        a->h = dlopen(want, RTLD_NOW | RTLD_LOCAL | RTLD_DEEPBIND);
        if (!a->h) {
            snprintf(a->error, sizeof a->error, "cannot load %s: %s", want, dlerror());
            return a;
        }
        bool ok = true;
        auto bind = [&](auto& fn, const char* name) {
            fn = reinterpret_cast<std::remove_reference_t<decltype(fn)>>(dlsym(a->h, name));
            if (!fn && ok) {
                snprintf(a->error, sizeof a->error, "%s has no %s", want, name);
                ok = false;
            }
        };
        bind(a->GetVersion, "ncclGetVersion");
        bind(a->GetErrorString, "ncclGetErrorString");
        bind(a->GetUniqueId, "ncclGetUniqueId");
        bind(a->CommInitRank, "ncclCommInitRank");
        bind(a->CommInitAll, "ncclCommInitAll");
        bind(a->CommDestroy, "ncclCommDestroy");
        bind(a->GroupStart, "ncclGroupStart");
        bind(a->GroupEnd, "ncclGroupEnd");
        bind(a->Send, "ncclSend");
        bind(a->Recv, "ncclRecv");
        if (!ok) {
            a->h = nullptr;   // unusable: every RCCL entry point fails with the error
            return a;
        }
        Dl_info info{};
        snprintf(a->path, sizeof a->path, "%s",
                 dladdr(reinterpret_cast<void*>(a->GetVersion), &info) && info.dli_fname ? info.dli_fname : want);
        return a;
    }();
    return *api;
}

#define RCCL_LOADED()                                                      \
    do {                                                                   \
        if (!rccl_api().h) return fail(MPX_ERR_RCCL, "%s", rccl_api().error); \
    } while (0)

#define NCCLCK(expr)                                                                                \
    do {                                                                                            \
        ncclResult_t r_ = (expr);                                                                   \
        if (r_ != ncclSuccess)                                                                      \
            return fail(MPX_ERR_RCCL, "%s:%d %s: %s", __FILE__, __LINE__, #expr, rccl_api().GetErrorString(r_)); \
    } while (0)

namespace {

unsigned char* slot_ptr(const Rank& rk, int j, int iters, int slots, long long len) {
    const int s = ring_slot(j, iters, slots);
    return s == 0 ? rk.rx : rk.ring + (long long)(s - 1) * len;
}

// the receives the reference's non-blocking loop completes (Waitall) for
// `iters` iterations: slot 255 of each full window is never waited for
// (mpi_perf.c:95-124)
u64 nb_waited(int iters) {
    return (u64)iters - (u64)(iters / kNbWindow);
}

// What the two stream engines share around their loops.  Begin: the checksum
// words zeroed (check mode), the status reset, the call's start time and
// start event.
int stream_begin(Rank& me, int check, int iters, double* t0) {
    if (check) HIPCK(hipMemsetAsync(me.csum, 0, (size_t)iters * sizeof(u64), me.stream));
    me.status->err = 0;
    me.status->where = 0;
    me.status->recv_done = 0;
    me.status->recv_digest = 0;
    *t0 = now_s();
    HIPCK(hipEventRecord(me.ev0, me.stream));
    return MPX_OK;
}

// End: the end event and the wait for it, the call's times, and its receive
// accounting — in check mode counted on the device (k_account), otherwise
// the loop's structure fixes the count.
int stream_end(Rank& me, int check, int mode, int iters, double t0, int launches, int protocol, mpx_timing* t) {
    HIPCK(hipEventRecord(me.ev1, me.stream));
    HIPCK(hipEventSynchronize(me.ev1));
    t->wall_s = now_s() - t0;
    float ms = 0;
    HIPCK(hipEventElapsedTime(&ms, me.ev0, me.ev1));
    t->device_s = ms * 1e-3;
    t->launches = launches;
    t->nwg = 0;
    t->protocol = protocol;
    t->recv_done = check ? __atomic_load_n(&me.status->recv_done, __ATOMIC_ACQUIRE)
                         : (mode == MPX_MODE_NONBLOCKING ? nb_waited(iters) : (u64)iters);
    t->recv_digest = __atomic_load_n(&me.status->recv_digest, __ATOMIC_ACQUIRE);
    return MPX_OK;
}

// check mode for the stream engines: checksum the received bytes into
// csum[i], then poison them — stream-ordered before the next push.
int stream_check(Rank& me, long long n, int i, int iters, unsigned char* buf = nullptr) {
    if (n <= 0) return MPX_OK;
    if (!buf) buf = me.rx;
    HIPCK(launch_checksum(buf, (size_t)n, me.csum + i, me.stream));
    if (i + 1 < iters)   // the last payload stays in rx, as in the reference
        HIPCK(launch_fill(buf, (size_t)n, MPX_FILL_BYTE, (0x5a ^ i) & 0xff, me.stream));
    return MPX_OK;
}

// What every operations object (mpx_stream_loop.h) has of its rank: the
// launches it counts, check mode's per-receive checksum, and the device-side
// receive accounting (neither counted).
struct RankOps {
    Rank& me;
    int launches = 0;   // mpx_timing.launches of the loop
    int check(long long n, int i, int iters) { return stream_check(me, n, i, iters); }
    int account(int j0, int count, long long n) {
        HIPCK(launch_account(me.status, me.csum, j0, count, n, me.stream));
        return MPX_OK;
    }
};

// ---------------------------------------------------------------------------
// engine: SDMA — hipMemcpyAsync into the peer's rx, then a one-lane flag
// store; the receiver's stream waits on its mailbox flag with a one-lane poll.
// ---------------------------------------------------------------------------
// The SDMA engine's payload copy kind.  Between two GPUs it is
// hipMemcpyDeviceToDeviceNoCU: the runtime must use a copy engine (SDMA), the
// engine north_star (b) names.  Within one GPU (loopback pairs) it is the
// plain device-to-device kind, which the runtime runs as its blit kernel on
// the CUs (profiles/r02_sdma_engine_loopback_kernel_stats.csv): two ranks of
// one GPU share its SDMA queues, and a copy waiting at the head of a shared
// queue for its own rank's poll blocks the other rank's copy behind it — the
// loopback ping-pong timed out that way with NoCU copies
// (profiles/r02_sdma_kind_ab.jsonl), which also moved 40 GB/s against the
// blit kernel's 570 on one GPU.  A rank paired with itself has one stream and
// cannot deadlock so.  MPX_SDMA_KIND=nocu|blit forces one kind (A/B).
hipMemcpyKind sdma_kind(const Rank& me, const Rank& peer) {
    static const int forced = [] {
        const char* v = getenv("MPX_SDMA_KIND");
        return !v ? 0 : !strcmp(v, "nocu") ? 1 : !strcmp(v, "blit") ? 2 : 0;
    }();
    const bool same_gpu = &me != &peer && same_device(me, peer);   // distinct ranks of one GPU
    const bool nocu = forced == 1 || (forced == 0 && !same_gpu);
    return nocu ? hipMemcpyDeviceToDeviceNoCU : hipMemcpyDeviceToDevice;
}

// The SDMA engine's primitives; each counts one launch when it enqueues.
// Push number i + 1 of the call is tx0 + i + 1 on this side's sends, rx0 +
// i + 1 on the peer's.
struct SdmaOps : RankOps {
    Rank& peer;
    int my_slot, peer_slot;
    u64 tmo;
    u64 tx0, rx0;               // the link's push numbers before the call
    const u64* txb = nullptr;   // graph capture: seqs relative to these device words
    const u64* rxb = nullptr;
    int copy(void* dst, const void* src, long long n, bool lost) {
        if (n <= 0 || lost) return MPX_OK;
        HIPCK(hipMemcpyAsync(dst, src, (size_t)n, sdma_kind(me, peer), me.stream));
        ++launches;
        return MPX_OK;
    }
    // The flag store is a one-lane kernel ordered after the copy on this
    // stream (hipStreamWriteValue64 measured slower, 10.9 vs 8.6 us per
    // iteration, profiles/r01_sdma_signal_ab.jsonl).  Waits are bounded
    // one-lane kernels: a stream-level wait (hipStreamWaitValue64) cannot
    // time out.  base: the capture's sequence base (txb / rxb), or null.
    int signal(u64* flag, const u64* base, u64 v) {
        HIPCK(launch_signal(flag, base, v, me.stream));
        ++launches;
        return MPX_OK;
    }
    int wait(const u64* flag, const u64* base, u64 v) {
        HIPCK(launch_wait(flag, base, v, me.status, tmo, me.stream));
        ++launches;
        return MPX_OK;
    }
};

// Pushed: a send copies tx into the peer's rx and, when `publish`, stores the
// push's number into the peer's flag; a receive waits for this rank's flag.
struct SdmaPush : SdmaOps {
    int send(long long n, int i, bool publish, bool lost, bool /*ack*/) {
        TRY(copy(peer.rx, me.tx, n, lost));
        return publish ? signal(&peer.mb->flag[my_slot][0], txb, tx0 + i + 1) : MPX_OK;
    }
    int recv(long long, int i, bool, bool, bool) { return wait(&me.mb->flag[peer_slot][0], rxb, rx0 + i + 1); }
    int nb_post(long long n, int i, bool publish, bool lost) { return send(n, i, publish, lost, false); }
    int nb_flush(int i, int) { return wait(&me.mb->flag[peer_slot][0], rxb, rx0 + i); }   // not slot 255's receive
    int drain(const StreamCall& c, int inflight) {                           // the final Waitall(inflight)
        return c.mode == MPX_MODE_NONBLOCKING && inflight > 0 ? nb_flush(c.iters, inflight) : MPX_OK;
    }
};

// Pulled (MPX_XFER_PULL; the kernel engine's k_xfer_pull in stream form).  A
// send publishes "tx holds push seq" in the peer's ready word (tx is read-only
// while the loop runs, and the reference re-sends the same buffer).  A receive
// waits for the peer's ready word, copies the peer's tx into rx on this rank's
// stream (a copy engine reading the peer's HBM across GPUs), then, when
// `publish`, hands the peer's tx back (credit = seq, for every push up to
// seq).  Unidir's 1-byte ack stays a push, and is never the lost payload.
struct SdmaPull : SdmaPush {
    int send(long long n, int i, bool, bool, bool ack) {
        if (ack) return SdmaPush::send(n, i, true, false, true);
        return signal(&peer.mb->ready[my_slot], txb, tx0 + i + 1);
    }
    int recv(long long n, int i, bool publish, bool lost, bool ack) {
        if (ack) return SdmaPush::recv(n, i, true, false, true);
        TRY(wait(&me.mb->ready[peer_slot], rxb, rx0 + i + 1));
        TRY(copy(me.rx, peer.tx, n, lost));
        return publish ? signal(&peer.mb->credit[my_slot][0], rxb, rx0 + i + 1) : MPX_OK;
    }
    // Isend + Irecv; the receive is complete on this stream once its copy
    // ran; credits go back on the push's publish schedule
    int nb_post(long long n, int i, bool publish, bool lost) {
        TRY(send(n, i, true, false, false));
        return recv(n, i, publish, lost, false);
    }
    // every one of this side's sends up to tx0 + i copied by the peer.
    // Waitall(255): the peer's copies of sends 0..254; the receives of slots
    // 0..254 are done (stream order)
    int nb_flush(int i, int) { return wait(&me.mb->credit[peer_slot][0], txb, tx0 + i); }
    // a side that sent B-byte payloads waits for the peer's copies of its tx
    int drain(const StreamCall& c, int) {
        return c.mode != MPX_MODE_UNIDIR || c.group == 1 ? nb_flush(c.iters, 0) : MPX_OK;
    }
};

// The non-blocking loop in check mode, stream-ordered (the kernel engine's
// k_xfer_nbcheck in host-enqueued form): receive i lands in slot ring_slot(i)
// of the receiver; before a push reuses a slot the sender's stream waits for
// the receiver's credit; each receive is waited for, checksummed and poisoned
// right after this side's push i (so the two streams never wait on each other
// in a cycle), then its slot is handed back (the credit), and the device
// counts the reference's Waitall receives (account at each flush).  The call's
// receives were posted (Mailbox.posted) before it starts, so the first `slots`
// pushes need no credit.  Sequence numbers are absolute: never captured.
struct SdmaNbChecked : SdmaPush {
    int iters, slots;
    int nb_post(long long n, int i, bool, bool lost) {
        if (i >= slots) TRY(wait(&me.mb->credit[peer_slot][0], nullptr, tx0 + (u64)(i - slots + 1)));
        TRY(copy(slot_ptr(peer, i, iters, slots, n), me.tx, n, lost));
        TRY(signal(&peer.mb->flag[my_slot][0], nullptr, tx0 + i + 1));
        return wait(&me.mb->flag[peer_slot][0], nullptr, rx0 + i + 1);
    }
    int check(long long n, int i, int) {
        TRY(stream_check(me, n, i, iters, slot_ptr(me, i, iters, slots, n)));
        return signal(&peer.mb->credit[my_slot][0], nullptr, rx0 + i + 1);
    }
    int nb_flush(int, int) { return MPX_OK; }   // every receive was waited for where it was checked
    int drain(const StreamCall&, int) { return MPX_OK; }
};

// Graph-captured chunks of the SDMA loop (no check mode): the host enqueues
// ~3 operations per iteration at ~3.5 us each, so the plain loop is
// host-bound (9.4-10.4 us per ping-pong iteration on a loopback pair, 6.0 us
// replayed, profiles/r01_sdma_graph_ab.jsonl); capture and instantiation
// happen before the timed region.  Sequence numbers in a chunk are relative to
// me.scratch[2..3], which k_seqbase sets before the first replay and each
// chunk's last node advances by its iteration count.  Full chunks have
// kSdmaChunk = 256 iterations, which keeps the non-blocking window (a flush
// every 256 iterations) aligned with them; the remainder (< 256, no flush
// inside) is one more captured chunk of its own length.
constexpr int kSdmaChunk = kNbWindow;
constexpr int kSdmaGraphMin = 16;   // fewer iterations: plain enqueue

bool sdma_graphs_enabled() {
    static const bool on = [] {
        const char* v = getenv("MPX_SDMA_GRAPH");
        return !(v && atoi(v) == 0);
    }();
    return on;
}

// what a call of `iters` iterations replays: full chunks, and the remainder
// if it is worth a graph (not in check mode, whose per-iteration checksum
// slots would move with every chunk)
struct SdmaSplit { int chunks, rest; };
SdmaSplit sdma_split(int iters, bool check) {
    if (check || !sdma_graphs_enabled() || iters < kSdmaGraphMin) return {0, 0};
    return {iters / kSdmaChunk, iters % kSdmaChunk >= kSdmaGraphMin ? iters % kSdmaChunk : 0};
}

int sdma_chunk_graph(Rank& me, Rank& peer, int my_rank, int peer_rank, int mode, int group, long long len,
                     u64 tmo, int count, hipGraphExec_t* out, bool pull = false) {
    const SdmaKey key{mode + (pull ? 8 : 0), group, peer_rank, len, tmo, count};
    auto it = me.sdma_graphs.find(key);
    if (it != me.sdma_graphs.end()) {
        *out = it->second;
        return MPX_OK;
    }
    const StreamCall c{mode, group, len, count, false, nb_publish(), 0};
    SdmaPush push{{{me}, peer, my_rank, peer_rank, tmo, 0, 0, me.scratch + kScrSeqBase, me.scratch + kScrSeqBase + 1}};
    SdmaPull pulled{push};
    HIPCK(hipStreamBeginCapture(me.stream, hipStreamCaptureModeThreadLocal));
    int inflight = 0;
    int st = pull ? stream_loop(pulled, c, 0, count, &inflight) : stream_loop(push, c, 0, count, &inflight);
    if (st == MPX_OK) st = launch_seqbase(me.scratch + kScrSeqBase, count, count, 1, me.stream) == hipSuccess
                               ? MPX_OK : fail(MPX_ERR_HIP, "k_seqbase launch in capture");
    hipGraph_t g = nullptr;
    const hipError_t e = hipStreamEndCapture(me.stream, &g);
    if (st != MPX_OK) {
        if (g) (void)hipGraphDestroy(g);
        return st;
    }
    HIPCK(e);
    hipGraphExec_t x = nullptr;
    const hipError_t ei = hipGraphInstantiate(&x, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    HIPCK(ei);
    me.sdma_graphs[key] = x;
    *out = x;
    return MPX_OK;
}

}  // namespace

int run_sdma(Rank& me, Rank& peer, int my_rank, int peer_rank, int mode, int group, int iters, long long len,
             const mpx_xfer_opts* o, mpx_timing* t, bool pull) {
    const int check = (o && o->check) ? 1 : 0;
    const int slots = link_slots(me, peer, len);
    const bool nbcheck = !pull && check && mode == MPX_MODE_NONBLOCKING;
    if (nbcheck && len > 0 && slots > 1 && (!me.ring || !peer.ring))
        return fail(MPX_ERR_STATE, "rank %d/%d: check-mode receive ring missing", my_rank, peer_rank);
    const u64 txs0 = me.tx_seq[peer_rank], rxs0 = me.rx_seq[peer_rank];
    const StreamCall c{mode, group, len, iters, check != 0, nb_publish(), test_knobs().skip_push};
    const SdmaPush push{{{me}, peer, my_rank, peer_rank, timeout_ticks(o), txs0, rxs0}};
    // graph-replayed chunks for the bulk of the loop
    const SdmaSplit sp = sdma_split(iters, check);
    hipGraphExec_t full = nullptr, tail = nullptr;
    if (sp.chunks > 0)
        TRY(sdma_chunk_graph(me, peer, my_rank, peer_rank, mode, group, len, push.tmo, kSdmaChunk, &full, pull));
    if (sp.rest > 0)
        TRY(sdma_chunk_graph(me, peer, my_rank, peer_rank, mode, group, len, push.tmo, sp.rest, &tail, pull));
    if (full || tail) HIPCK(launch_seqbase(me.scratch + kScrSeqBase, txs0, rxs0, 0, me.stream));
    double t0 = 0;
    TRY(stream_begin(me, check, iters, &t0));
    int launches = 0;
    auto enqueue = [&](auto op) -> int {
        // matched-receive order (Mailbox.posted), stream-ordered: post this
        // call's receives, and a side that pushes first waits for the peer's
        // post before its first copy into the peer's rx
        if (iters > 0 && !test_knobs().no_posted) {
            const u64 call = ++me.calls[peer_rank];
            TRY(op.signal(&peer.mb->posted[my_rank], nullptr, call));
            if (mode == MPX_MODE_NONBLOCKING || group == 1) TRY(op.wait(&me.mb->posted[peer_rank], nullptr, call));
        }
        for (int k = 0; k < sp.chunks; ++k) HIPCK(hipGraphLaunch(full, me.stream));
        if (tail) HIPCK(hipGraphLaunch(tail, me.stream));
        const int replayed = sp.chunks * kSdmaChunk + sp.rest;
        int inflight = replayed % kSdmaChunk;   // the window a replayed remainder leaves open
        TRY(stream_loop(op, c, replayed, iters, &inflight));
        TRY(stream_tail(op, c, inflight));
        launches = op.launches + sp.chunks + (tail ? 1 : 0);   // graph replays count once each
        return MPX_OK;
    };
    TRY(nbcheck ? enqueue(SdmaNbChecked{push, iters, slots}) : pull ? enqueue(SdmaPull{push}) : enqueue(push));
    TRY(stream_end(me, check, mode, iters, t0, launches, pull ? kProtoSdmaPull : kProtoSdma, t));
    if (__atomic_load_n(&me.status->err, __ATOMIC_ACQUIRE)) {
        me.broken = true;
        return fail(MPX_ERR_TIMEOUT, "rank %d <- rank %d: SDMA-engine wait timed out (flag %llu, awaited %llu; "
                    "sequence bases tx %llu rx %llu, mode %d, %lld B, %d iterations)", my_rank, peer_rank,
                    me.status->seen, me.status->want, txs0, rxs0, mode, len, iters);
    }
    me.tx_seq[peer_rank] += (u64)iters;
    me.rx_seq[peer_rank] += (u64)iters;
    return MPX_OK;
}

// ---------------------------------------------------------------------------
// engine: RCCL — ncclSend/ncclRecv on the rank's stream: 2 launches per
// blocking iteration, 1 per non-blocking group
// ---------------------------------------------------------------------------
namespace {
struct RcclOps : RankOps {
    int peer_rank;
    int send(long long len, int, bool, bool lost, bool) {
        // test knob: the "lost" send carries rx (poison or stale bytes), not tx
        const void* src = lost ? (const void*)me.rx : (const void*)me.tx;
        const size_t n = (size_t)len;
        NCCLCK(rccl_api().Send(src, n, ncclChar, peer_rank, me.comm, me.stream));
        ++launches;
        return MPX_OK;
    }
    int recv(long long len, int, bool, bool, bool) {
        const size_t n = (size_t)len;
        NCCLCK(rccl_api().Recv(me.rx, n, ncclChar, peer_rank, me.comm, me.stream));
        ++launches;
        return MPX_OK;
    }
    // Isend + Irecv of one iteration: one fused group (full duplex).  Check
    // mode: the receive lands in rx and is checksummed (and poisoned) on this
    // stream before the next group's receive can land — RCCL writes only this
    // rank's own buffer, so no slots or credits are needed; the device counts
    // the Waitall receives.
    int nb_post(long long len, int, bool, bool lost) {
        const void* src = lost ? (const void*)me.rx : (const void*)me.tx;
        const size_t n = (size_t)len;
        NCCLCK(rccl_api().GroupStart());
        NCCLCK(rccl_api().Send(src, n, ncclChar, peer_rank, me.comm, me.stream));
        NCCLCK(rccl_api().Recv(me.rx, n, ncclChar, peer_rank, me.comm, me.stream));
        NCCLCK(rccl_api().GroupEnd());
        ++launches;
        return MPX_OK;
    }
    int nb_flush(int, int) { return MPX_OK; }   // stream order completes every receive
    int drain(const StreamCall&, int) { return MPX_OK; }
};
}  // namespace

int run_rccl(Rank& me, Rank& peer, int my_rank, int peer_rank, int mode, int group, int iters, long long len,
             const mpx_xfer_opts* o, mpx_timing* t) {
    (void)peer;
    if (!me.comm) return fail(MPX_ERR_STATE, "rank %d has no RCCL communicator (mpx_rccl_init_*)", my_rank);
    const int check = (o && o->check) ? 1 : 0;
    const StreamCall c{mode, group, len, iters, check != 0, nb_publish(), test_knobs().skip_push};
    double t0 = 0;
    TRY(stream_begin(me, check, iters, &t0));
    RcclOps op{{me}, peer_rank};
    int inflight = 0;
    TRY(stream_loop(op, c, 0, iters, &inflight));
    TRY(stream_tail(op, c, inflight));
    return stream_end(me, check, mode, iters, t0, op.launches, kProtoRccl, t);
}

}  // namespace mpx

extern "C" {

namespace {
// RCCL connects a pair lazily, on its first send/receive: transport setup and
// the exchange of buffer handles, milliseconds across GPUs.  The reference's
// MPI does the same, and its record of run 0 — the only run that pays it in a
// reference job — is dropped (mpi_perf.c:545).  In all-pairs rounds every
// round meets new peers, so runs 1..N-2 would carry that setup inside their
// recorded time; a one-byte exchange here, once per pair, before the barrier,
// takes it out.  Both ranks of the pair call it (as they call the transfer),
// on the rank's stream, into scratch words no transfer uses.
int rccl_link(Rank& me, int my_rank, int peer_rank) {
    if (!me.comm) return fail(MPX_ERR_STATE, "rank %d has no RCCL communicator (mpx_rccl_init_*)", my_rank);
    if (me.rccl_linked[peer_rank]) return MPX_OK;
    DeviceGuard g(me.dev);
    HIPCK(g.err);
    NCCLCK(rccl_api().GroupStart());
    NCCLCK(rccl_api().Send(me.scratch + kScrLink, 1, ncclChar, peer_rank, me.comm, me.stream));
    NCCLCK(rccl_api().Recv(me.scratch + kScrLink + 1, 1, ncclChar, peer_rank, me.comm, me.stream));
    NCCLCK(rccl_api().GroupEnd());
    HIPCK(hipStreamSynchronize(me.stream));
    me.rccl_linked[peer_rank] = true;
    return MPX_OK;
}
}  // namespace

int mpx_xfer_prepare(mpx_ctx* ctx, int mode, int my_group, int my_rank, int peer_rank, int iters, int buff_len,
                     const mpx_xfer_opts* opts) {
    if (!ctx) return fail(MPX_ERR_INVALID, "NULL argument");
    TRY(check_args(ctx, mode, nullptr, my_rank, peer_rank, iters, buff_len));
    Rank& me = ctx->r[my_rank];
    Rank& peer = ctx->r[peer_rank];
    if (!me.local) return fail(MPX_ERR_STATE, "rank %d is not attached in this process", my_rank);
    if (ctx->engine == MPX_ENGINE_RCCL) return rccl_link(me, my_rank, peer_rank);
    // the SDMA engine builds its graph-captured chunks per (mode, side, peer,
    // B): what run_sdma replays (not used in check mode)
    const SdmaSplit sp = sdma_split(iters, opts && opts->check);
    if (ctx->engine != MPX_ENGINE_SDMA || (sp.chunks == 0 && sp.rest == 0)) return MPX_OK;
    if (!peer.local && !peer.imported) return fail(MPX_ERR_STATE, "peer rank %d is unknown", peer_rank);
    const bool pull = pull_requested(opts);   // pulled chunks copy from the peer's tx: mapped first
    if (pull && buff_len > 0 && !peer.tx) TRY(ensure_peer_tx(ctx, peer, peer_rank));
    DeviceGuard g(me.dev);
    HIPCK(g.err);
    const u64 tmo = timeout_ticks(opts);
    hipGraphExec_t x = nullptr;
    if (sp.chunks > 0)
        TRY(sdma_chunk_graph(me, peer, my_rank, peer_rank, mode, my_group, buff_len, tmo, kSdmaChunk, &x, pull));
    if (sp.rest > 0)
        TRY(sdma_chunk_graph(me, peer, my_rank, peer_rank, mode, my_group, buff_len, tmo, sp.rest, &x, pull));
    return MPX_OK;
}

int mpx_rccl_version(int* version, char* path, int len) {
    if (!version || !path || len < 64) return fail(MPX_ERR_INVALID, "bad argument");
    RCCL_LOADED();
    NCCLCK(rccl_api().GetVersion(version));
    snprintf(path, (size_t)len, "%s", rccl_api().path);
    return MPX_OK;
}

int mpx_rccl_get_unique_id(void* id) {
    if (!id) return fail(MPX_ERR_INVALID, "id is NULL");
    static_assert(sizeof(ncclUniqueId) == MPX_RCCL_ID_BYTES, "RCCL unique id size");
    RCCL_LOADED();
    ncclUniqueId u;
    NCCLCK(rccl_api().GetUniqueId(&u));
    memcpy(id, &u, sizeof u);
    return MPX_OK;
}

int mpx_rccl_init_rank(mpx_ctx* ctx, int rank, int nranks, const void* id) {
    if (!ctx || !id) return fail(MPX_ERR_INVALID, "NULL argument");
    if (rank < 0 || rank >= ctx->nranks || !ctx->r[rank].local) return fail(MPX_ERR_STATE, "rank %d is not attached", rank);
    Rank& rk = ctx->r[rank];
    if (rk.comm) return fail(MPX_ERR_STATE, "rank %d already has a communicator", rank);
    RCCL_LOADED();
    DeviceGuard g(rk.dev);
    HIPCK(g.err);
    ncclUniqueId u;
    memcpy(&u, id, sizeof u);
    NCCLCK(rccl_api().CommInitRank(&rk.comm, nranks, u, rank));
    rk.comm_rank = rank;
    return MPX_OK;
}

int mpx_rccl_init_all(mpx_ctx* ctx) {
    if (!ctx) return fail(MPX_ERR_INVALID, "ctx is NULL");
    std::vector<int> devs;
    for (int i = 0; i < ctx->nranks; ++i) {
        if (!ctx->r[i].local) return fail(MPX_ERR_STATE, "rank %d is not attached locally", i);
        if (ctx->r[i].comm) return fail(MPX_ERR_STATE, "rank %d already has a communicator", i);
        devs.push_back(ctx->r[i].dev);
    }
    RCCL_LOADED();
    std::vector<ncclComm_t> comms(devs.size());
    NCCLCK(rccl_api().CommInitAll(comms.data(), (int)devs.size(), devs.data()));
    for (int i = 0; i < ctx->nranks; ++i) {
        ctx->r[i].comm = comms[i];
        ctx->r[i].comm_rank = i;
    }
    return MPX_OK;
}

}  // extern "C"
