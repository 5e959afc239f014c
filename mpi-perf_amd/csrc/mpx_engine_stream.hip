// mpx_engine_stream.hip — the two stream engines behind mpx_xfer_ex: SDMA
// (run_sdma) and RCCL (run_rccl, with its run-time loader and the mpx_rccl_*
// entry points), and what prepares them ahead of a call (mpx_xfer_prepare).
// Both enqueue their loop on the rank's stream between one begin
// (stream_begin) and one end (stream_end).
#include "mpx_runtime.h"

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

// ---------------------------------------------------------------------------
// engine: SDMA — hipMemcpyAsync into the peer's rx, then a one-lane flag
// store; the receiver's stream waits on its mailbox flag with a one-lane poll.
// ---------------------------------------------------------------------------
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
hipMemcpyKind sdma_kind(bool same_gpu) {
    static const int forced = [] {
        const char* v = getenv("MPX_SDMA_KIND");
        return !v ? 0 : !strcmp(v, "nocu") ? 1 : !strcmp(v, "blit") ? 2 : 0;
    }();
    const bool nocu = forced == 1 || (forced == 0 && !same_gpu);
    return nocu ? hipMemcpyDeviceToDeviceNoCU : hipMemcpyDeviceToDevice;
}

// non-blocking publish schedule shared by the kernel and SDMA engines: every
// nb_publish() pushes, at window slot 254 (the last receive a Waitall(255)
// waits for, so no flush waits for the slot-255 push the reference leaves
// pending) and at the last push
bool nb_publishes(int i, int iters) {
    return (i + 1) % nb_publish() == 0 || i % kNbWindow == kNbWindow - 2 || i + 1 == iters;
}

struct SdmaOps {
    Rank& me;
    Rank& peer;
    int my_slot, peer_slot;
    u64 tmo;
    const u64* txb = nullptr;   // graph capture: seqs relative to these device words
    const u64* rxb = nullptr;
    int launches = 0;
    int skip = 0;               // test knob: 1 + iteration whose copy is skipped
    bool pull = false;          // MPX_XFER_PULL: B-byte payloads copied by the receiver's stream
    // The flag store is a one-lane kernel ordered after the copy on this
    // stream (hipStreamWriteValue64 measured slower, 10.9 vs 8.6 us per
    // iteration, profiles/r01_sdma_signal_ab.jsonl).  Waits are bounded
    // one-lane kernels: a stream-level wait (hipStreamWaitValue64) cannot
    // time out.
    int push(long long n, u64 seq, bool publish = true, bool skip_copy = false) {
        if (n > 0 && !skip_copy) {
            HIPCK(hipMemcpyAsync(peer.rx, me.tx, (size_t)n, sdma_kind(&me != &peer && same_device(me, peer)),
                                 me.stream));
            ++launches;
        }
        if (!publish) return MPX_OK;
        HIPCK(launch_signal(&peer.mb->flag[my_slot][0], txb, seq, me.stream));
        ++launches;
        return MPX_OK;
    }
    int wait(u64 seq) {
        HIPCK(launch_wait(&me.mb->flag[peer_slot][0], rxb, seq, me.status, tmo, me.stream));
        ++launches;
        return MPX_OK;
    }
    // Pull mode (the kernel engine's k_xfer_pull in stream form).  A send
    // publishes "tx holds push seq" in the peer's ready word (tx is read-only
    // while the loop runs, and the reference re-sends the same buffer).
    int pull_send(u64 seq) {
        HIPCK(launch_signal(&peer.mb->ready[my_slot], txb, seq, me.stream));
        ++launches;
        return MPX_OK;
    }
    // A receive waits for the peer's ready word, copies the peer's tx into rx
    // on this rank's stream (a copy engine reading the peer's HBM across
    // GPUs), then, when `publish`, hands the peer's tx back (credit = seq,
    // for every push up to seq).
    int pull_recv(long long n, u64 seq, bool publish, bool skip_copy) {
        HIPCK(launch_wait(&me.mb->ready[peer_slot], rxb, seq, me.status, tmo, me.stream));
        ++launches;
        if (n > 0 && !skip_copy) {
            HIPCK(hipMemcpyAsync(me.rx, peer.tx, (size_t)n, sdma_kind(&me != &peer && same_device(me, peer)),
                                 me.stream));
            ++launches;
        }
        if (!publish) return MPX_OK;
        HIPCK(launch_signal(&peer.mb->credit[my_slot][0], rxb, seq, me.stream));
        ++launches;
        return MPX_OK;
    }
    // every one of this side's sends up to `seq` copied by the peer
    int wait_pulled(u64 seq) {
        HIPCK(launch_wait(&me.mb->credit[peer_slot][0], txb, seq, me.status, tmo, me.stream));
        ++launches;
        return MPX_OK;
    }
    // one iteration of the pulled loop (see step)
    int pull_step(int mode, int group, long long len, int i, int iters, u64 tx0, u64 rx0, bool check, int* inflight) {
        const bool sk = skip == i + 1;
        if (mode == MPX_MODE_PINGPONG) {
            if (group == 1) {
                TRY(pull_send(tx0 + i + 1));
                TRY(pull_recv(len, rx0 + i + 1, true, sk));
                if (check) TRY(stream_check(me, len, i, iters));
            } else {
                TRY(pull_recv(len, rx0 + i + 1, true, sk));
                if (check) TRY(stream_check(me, len, i, iters));
                TRY(pull_send(tx0 + i + 1));
            }
        } else if (mode == MPX_MODE_UNIDIR) {
            if (group == 1) {
                TRY(pull_send(tx0 + i + 1));
                TRY(wait(rx0 + i + 1));                      // the 1-byte ack, pushed
                if (check) TRY(stream_check(me, 1, i, iters));
            } else {
                TRY(pull_recv(len, rx0 + i + 1, true, sk));
                if (check) TRY(stream_check(me, len, i, iters));
                TRY(push(1, tx0 + i + 1, true, false));      // Send(tx, 1): always one byte, pushed
            }
        } else {
            // Isend + Irecv; the receive is complete on this stream once its
            // copy ran; credits go back on the push's publish schedule
            TRY(pull_send(tx0 + i + 1));
            TRY(pull_recv(len, rx0 + i + 1, nb_publishes(i, iters), sk));
            if (check) TRY(stream_check(me, len, i, iters));
            if (*inflight == kNbWindow - 1) {
                // Waitall(255): the peer's copies of sends 0..254; the
                // receives of slots 0..254 are done (stream order) — count them
                TRY(wait_pulled(tx0 + i));
                if (check) HIPCK(launch_account(me.status, me.csum, i - *inflight, *inflight, len, me.stream));
                *inflight = 0;
            } else {
                ++*inflight;
            }
        }
        return MPX_OK;
    }
    // one iteration i of the loop (mpi_perf.c:70-82, 95-124, 132-144), seqs
    // relative to tx0 / rx0; check mode checksums + poisons each received
    // payload where the reference's Recv returns (before the reply / ack);
    // *inflight is the non-blocking window fill
    int step(int mode, int group, long long len, int i, int iters, u64 tx0, u64 rx0, bool check, int* inflight) {
        if (pull) return pull_step(mode, group, len, i, iters, tx0, rx0, check, inflight);
        const bool sk = skip == i + 1;
        if (mode == MPX_MODE_PINGPONG) {
            if (group == 1) {
                TRY(push(len, tx0 + i + 1, true, sk));
                TRY(wait(rx0 + i + 1));
                if (check) TRY(stream_check(me, len, i, iters));
            } else {
                TRY(wait(rx0 + i + 1));
                if (check) TRY(stream_check(me, len, i, iters));
                TRY(push(len, tx0 + i + 1, true, sk));
            }
        } else if (mode == MPX_MODE_UNIDIR) {
            if (group == 1) {
                TRY(push(len, tx0 + i + 1, true, sk));
                TRY(wait(rx0 + i + 1));
                if (check) TRY(stream_check(me, 1, i, iters));
            } else {
                TRY(wait(rx0 + i + 1));
                if (check) TRY(stream_check(me, len, i, iters));
                TRY(push(1, tx0 + i + 1, true, sk));        // Send(tx, 1): always one byte
            }
        } else {
            TRY(push(len, tx0 + i + 1, nb_publishes(i, iters), sk));
            if (*inflight == kNbWindow - 1) {
                TRY(wait(rx0 + i));                          // Waitall(255): not slot 255's receive
                *inflight = 0;
            } else {
                ++*inflight;
            }
        }
        return MPX_OK;
    }

    // The non-blocking loop in check mode, stream-ordered (the kernel
    // engine's k_xfer_nbcheck in host-enqueued form): receive i lands in slot
    // ring_slot(i) of the receiver; before a push reuses a slot the sender's
    // stream waits for the receiver's credit; each receive is waited for,
    // checksummed and poisoned right after this side's push i (so the two
    // streams never wait on each other in a cycle), and the device counts
    // the reference's Waitall receives (k_account at each flush).
    // The call's receives were posted (Mailbox.posted) before it starts, so
    // the first `slots` pushes need no credit.
    int nb_checked(int iters, long long len, u64 tx0, u64 rx0, int slots) {
        u64* credit_out = &peer.mb->credit[my_slot][0];
        const u64* credit_in = &me.mb->credit[peer_slot][0];
        int inflight = 0;
        for (int i = 0; i < iters; ++i) {
            if (i >= slots) TRY(wait_abs(credit_in, tx0 + (u64)(i - slots + 1)));
            if (len > 0 && skip != i + 1) {
                HIPCK(hipMemcpyAsync(slot_ptr(peer, i, iters, slots, len), me.tx, (size_t)len,
                                     sdma_kind(same_device(me, peer) && &me != &peer), me.stream));
                ++launches;
            }
            TRY(signal_abs(&peer.mb->flag[my_slot][0], tx0 + i + 1));
            TRY(wait_abs(&me.mb->flag[peer_slot][0], rx0 + i + 1));
            TRY(stream_check(me, len, i, iters, slot_ptr(me, i, iters, slots, len)));
            TRY(signal_abs(credit_out, rx0 + i + 1));
            if (inflight == kNbWindow - 1) {          // Waitall(255): iterations i-255 .. i-1
                HIPCK(launch_account(me.status, me.csum, i - inflight, inflight, len, me.stream));
                inflight = 0;
            } else {
                ++inflight;
            }
        }
        if (inflight > 0) HIPCK(launch_account(me.status, me.csum, iters - inflight, inflight, len, me.stream));
        return MPX_OK;
    }
    int signal_abs(u64* flag, u64 v) {
        HIPCK(launch_signal(flag, nullptr, v, me.stream));
        ++launches;
        return MPX_OK;
    }
    int wait_abs(const u64* flag, u64 v) {
        HIPCK(launch_wait(flag, nullptr, v, me.status, tmo, me.stream));
        ++launches;
        return MPX_OK;
    }
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

int sdma_chunk_graph(Rank& me, Rank& peer, int my_rank, int peer_rank, int mode, int group, long long len,
                     u64 tmo, int count, hipGraphExec_t* out, bool pull = false) {
    const SdmaKey key{mode + (pull ? 8 : 0), group, peer_rank, len, tmo, count};
    auto it = me.sdma_graphs.find(key);
    if (it != me.sdma_graphs.end()) {
        *out = it->second;
        return MPX_OK;
    }
    SdmaOps cap{me, peer, my_rank, peer_rank, tmo, me.scratch + kScrSeqBase, me.scratch + kScrSeqBase + 1};
    cap.pull = pull;
    HIPCK(hipStreamBeginCapture(me.stream, hipStreamCaptureModeThreadLocal));
    int inflight = 0, st = MPX_OK;
    for (int j = 0; j < count && st == MPX_OK; ++j) st = cap.step(mode, group, len, j, count, 0, 0, false, &inflight);
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
    SdmaOps op{me, peer, my_rank, peer_rank, timeout_ticks(o)};
    op.skip = test_knobs().skip_push;
    op.pull = pull;
    const int check = (o && o->check) ? 1 : 0;
    const int slots = link_slots(me, peer, len);
    if (!pull && check && mode == MPX_MODE_NONBLOCKING && len > 0 && slots > 1 && (!me.ring || !peer.ring))
        return fail(MPX_ERR_STATE, "rank %d/%d: check-mode receive ring missing", my_rank, peer_rank);
    const u64 txs0 = me.tx_seq[peer_rank], rxs0 = me.rx_seq[peer_rank];
    // graph-replayed chunks for the bulk of the loop (not in check mode,
    // whose per-iteration checksum slots would move with every chunk)
    const bool graphs = !check && sdma_graphs_enabled() && iters >= kSdmaGraphMin;
    const int chunks = graphs ? iters / kSdmaChunk : 0;
    const int rest = graphs && iters % kSdmaChunk >= kSdmaGraphMin ? iters % kSdmaChunk : 0;
    hipGraphExec_t full = nullptr, tail = nullptr;
    if (chunks > 0)
        TRY(sdma_chunk_graph(me, peer, my_rank, peer_rank, mode, group, len, op.tmo, kSdmaChunk, &full, pull));
    if (rest > 0) TRY(sdma_chunk_graph(me, peer, my_rank, peer_rank, mode, group, len, op.tmo, rest, &tail, pull));
    if (full || tail) HIPCK(launch_seqbase(me.scratch + kScrSeqBase, txs0, rxs0, 0, me.stream));
    double t0 = 0;
    TRY(stream_begin(me, check, iters, &t0));
    // matched-receive order (Mailbox.posted), stream-ordered: post this
    // call's receives, and a side that pushes first waits for the peer's
    // post before its first copy into the peer's rx
    if (iters > 0 && !test_knobs().no_posted) {
        const u64 call = ++me.calls[peer_rank];
        TRY(op.signal_abs(&peer.mb->posted[my_rank], call));
        if (mode == MPX_MODE_NONBLOCKING || group == 1) TRY(op.wait_abs(&me.mb->posted[peer_rank], call));
    }
    if (check && mode == MPX_MODE_NONBLOCKING && !pull) {
        TRY(op.nb_checked(iters, len, txs0, rxs0, slots));
    } else {
        for (int c = 0; c < chunks; ++c) HIPCK(hipGraphLaunch(full, me.stream));
        if (tail) HIPCK(hipGraphLaunch(tail, me.stream));
        int inflight = 0;
        const int replayed = chunks * kSdmaChunk + rest;
        for (int i = replayed; i < iters; ++i) TRY(op.step(mode, group, len, i, iters, txs0, rxs0, check, &inflight));
        if (pull) {
            // pulled: every receive is complete on this stream; the final
            // Waitall's receives are counted (check mode), and a side that
            // sent B-byte payloads waits for the peer's copies of its tx
            if (mode == MPX_MODE_NONBLOCKING && check && inflight > 0)
                HIPCK(launch_account(me.status, me.csum, iters - inflight, inflight, len, me.stream));
            if (iters > 0 && (mode != MPX_MODE_UNIDIR || group == 1)) TRY(op.wait_pulled(txs0 + iters));
        } else if (mode == MPX_MODE_NONBLOCKING && iters > 0 && (iters % kNbWindow) != 0) {
            TRY(op.wait(rxs0 + iters));
        }
        // every receive of ping-pong / unidir is complete here; the device
        // counts them and digests their checksums
        if (check && iters > 0 && mode != MPX_MODE_NONBLOCKING)
            HIPCK(launch_account(me.status, me.csum, 0, iters,
                                 (mode == MPX_MODE_UNIDIR && group == 1) ? 1 : len, me.stream));
    }
    // graph replays count once each
    TRY(stream_end(me, check, mode, iters, t0, op.launches + (chunks + (tail ? 1 : 0)),
                   pull ? kProtoSdmaPull : kProtoSdma, t));
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
// engine: RCCL — ncclSend/ncclRecv on the rank's stream
// ---------------------------------------------------------------------------
int run_rccl(Rank& me, Rank& peer, int my_rank, int peer_rank, int mode, int group, int iters, long long len,
             const mpx_xfer_opts* o, mpx_timing* t) {
    (void)peer;
    (void)my_rank;
    if (!me.comm) return fail(MPX_ERR_STATE, "rank %d has no RCCL communicator (mpx_rccl_init_*)", my_rank);
    const int check = (o && o->check) ? 1 : 0;
    const size_t n = (size_t)len;
    const int skip = test_knobs().skip_push;
    double t0 = 0;
    TRY(stream_begin(me, check, iters, &t0));
    int launches = 0, inflight = 0;
    for (int i = 0; i < iters; ++i) {
        // test knob: the "lost" send carries rx (poison or stale bytes), not tx
        const void* src = skip == i + 1 ? (const void*)me.rx : (const void*)me.tx;
        if (mode == MPX_MODE_PINGPONG) {
            if (group == 1) {
                NCCLCK(rccl_api().Send(src, n, ncclChar, peer_rank, me.comm, me.stream));
                NCCLCK(rccl_api().Recv(me.rx, n, ncclChar, peer_rank, me.comm, me.stream));
                if (check) TRY(stream_check(me, len, i, iters));
            } else {
                NCCLCK(rccl_api().Recv(me.rx, n, ncclChar, peer_rank, me.comm, me.stream));
                if (check) TRY(stream_check(me, len, i, iters));
                NCCLCK(rccl_api().Send(src, n, ncclChar, peer_rank, me.comm, me.stream));
            }
            launches += 2;
        } else if (mode == MPX_MODE_UNIDIR) {
            if (group == 1) {
                NCCLCK(rccl_api().Send(src, n, ncclChar, peer_rank, me.comm, me.stream));
                NCCLCK(rccl_api().Recv(me.rx, 1, ncclChar, peer_rank, me.comm, me.stream));
                if (check) TRY(stream_check(me, 1, i, iters));
            } else {
                NCCLCK(rccl_api().Recv(me.rx, n, ncclChar, peer_rank, me.comm, me.stream));
                if (check) TRY(stream_check(me, len, i, iters));
                NCCLCK(rccl_api().Send(src, 1, ncclChar, peer_rank, me.comm, me.stream));
            }
            launches += 2;
        } else {
            // Isend + Irecv of one iteration: one fused group (full duplex).
            // Check mode: the receive lands in rx and is checksummed (and
            // poisoned) on this stream before the next group's receive can
            // land — RCCL writes only this rank's own buffer, so no slots or
            // credits are needed; the device counts the Waitall receives.
            NCCLCK(rccl_api().GroupStart());
            NCCLCK(rccl_api().Send(src, n, ncclChar, peer_rank, me.comm, me.stream));
            NCCLCK(rccl_api().Recv(me.rx, n, ncclChar, peer_rank, me.comm, me.stream));
            NCCLCK(rccl_api().GroupEnd());
            launches += 1;
            if (check) {
                TRY(stream_check(me, len, i, iters));
                if (inflight == kNbWindow - 1) {       // Waitall(255): iterations i-255 .. i-1
                    HIPCK(launch_account(me.status, me.csum, i - inflight, inflight, len, me.stream));
                    inflight = 0;
                } else {
                    ++inflight;
                }
            }
        }
    }
    if (check && mode == MPX_MODE_NONBLOCKING && inflight > 0)
        HIPCK(launch_account(me.status, me.csum, iters - inflight, inflight, len, me.stream));
    if (check && mode != MPX_MODE_NONBLOCKING && iters > 0)
        HIPCK(launch_account(me.status, me.csum, 0, iters, (mode == MPX_MODE_UNIDIR && group == 1) ? 1 : len,
                             me.stream));
    return stream_end(me, check, mode, iters, t0, launches, kProtoRccl, t);
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
    if (mode < MPX_MODE_PINGPONG || mode > MPX_MODE_UNIDIR) return fail(MPX_ERR_INVALID, "mode %d", mode);
    if (my_rank < 0 || my_rank >= ctx->nranks || peer_rank < 0 || peer_rank >= ctx->nranks)
        return fail(MPX_ERR_INVALID, "ranks %d/%d", my_rank, peer_rank);
    if (iters < 0 || buff_len < 0) return fail(MPX_ERR_INVALID, "iters %d, buff_len %d", iters, buff_len);
    Rank& me = ctx->r[my_rank];
    Rank& peer = ctx->r[peer_rank];
    if (!me.local) return fail(MPX_ERR_STATE, "rank %d is not attached in this process", my_rank);
    if (ctx->engine == MPX_ENGINE_RCCL) return rccl_link(me, my_rank, peer_rank);
    // the SDMA engine builds its graph-captured chunks per (mode, side, peer,
    // B): what run_sdma replays (not used in check mode)
    if (ctx->engine != MPX_ENGINE_SDMA || (opts && opts->check) || !sdma_graphs_enabled() || iters < kSdmaGraphMin)
        return MPX_OK;
    if (!peer.local && !peer.imported) return fail(MPX_ERR_STATE, "peer rank %d is unknown", peer_rank);
    const bool pull = pull_requested(opts);   // pulled chunks copy from the peer's tx: mapped first
    if (pull && buff_len > 0 && !peer.tx) TRY(ensure_peer_tx(ctx, peer, peer_rank));
    DeviceGuard g(me.dev);
    HIPCK(g.err);
    const u64 tmo = timeout_ticks(opts);
    hipGraphExec_t x = nullptr;
    if (iters / kSdmaChunk > 0)
        TRY(sdma_chunk_graph(me, peer, my_rank, peer_rank, mode, my_group, buff_len, tmo, kSdmaChunk, &x, pull));
    if (iters % kSdmaChunk >= kSdmaGraphMin)
        TRY(sdma_chunk_graph(me, peer, my_rank, peer_rank, mode, my_group, buff_len, tmo, iters % kSdmaChunk, &x,
                             pull));
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
