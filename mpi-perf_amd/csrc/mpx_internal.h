// mpx_internal.h — types shared by the libmpx host side (mpx_runtime.hip,
// mpx_engine_kernel.hip, mpx_engine_stream.hip; their own shared declarations
// are in mpx_runtime.h) and its device code (mpx_kernels.hip).  Not part of
// the C-ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "../../include/mpx.h"

typedef unsigned long long u64;

// returns a status other than MPX_OK to the caller
#define TRY(expr)                     \
    do {                              \
        int s_ = (expr);              \
        if (s_ != MPX_OK) return s_;  \
    } while (0)

namespace mpx {

constexpr int kBlock = 256;              // threads per workgroup = 4 wave64
constexpr int kMaxPushWG = 256;          // flag slots per (receiver, sender) link
constexpr int kLLMaxBytes = 8192;        // messages <= this go as LL granules
constexpr int kLLGranules = kLLMaxBytes / 4;   // 4 payload bytes per granule
constexpr int kNbWindow = 256;           // MAX_REQ_NUM, mpi_perf.c:88
constexpr int kStageMaxBytes = 60 << 10; // LDS-staged tx chunk per workgroup, max
                                         // (under a 64 KiB per-workgroup LDS limit)

// Protocol ids reported in mpx_timing.protocol
enum Proto { kProtoLL = 0, kProtoBulk = 1, kProtoSdma = 2, kProtoRccl = 3, kProtoCopy = 4, kProtoCopySteps = 5,
             kProtoCopyPipe = 6, kProtoPull = 7, kProtoSdmaPull = 8, kProtoFan = 9, kProtoFanLL = 10, kProtoHostLL = 11,
             kProtoHostBulk = 12, kProtoHostDuplex = 13 };

// One rank's receive mailbox, in that rank's HBM (uncached / fine-grained so a
// poll sees stores that arrive over xGMI).  Written ONLY by the peers, polled
// only by the owner.
//   flag[s][w]   : sequence number of the last bulk push workgroup w of sender
//                  rank s finished into this rank's rx (written with one
//                  system-scope store after that workgroup's payload drained)
//   ll[s][g]     : LL granule g of the current small message from sender s:
//                  {tag:32 | payload:32}, tag = ll_tag(seq), one 8-byte store
//   credit[s][w] : sequence number of the last of THIS rank's pushes whose
//                  chunk w rank s is done with: non-blocking check mode —
//                  checksummed (and poisoned), i.e. the ring slot it used is
//                  free again; pull mode — loaded from this rank's tx, i.e.
//                  that chunk of tx may change again
//   ready[s]     : pull mode (MPX_XFER_PULL) — sequence number of the last
//                  push rank s made available in its tx (one store per send,
//                  by the sender; the receiver loads the bytes itself)
//   posted[s]    : "receives posted", written by rank s: the number of the
//                  latest transfer call between s and this rank that s has
//                  started.  It grows by one per call on both sides
//                  (Rank.calls), so no call's value equals an earlier call's.
//                  Rank s stores it as the first action of its call (its
//                  stream has then finished all of its previous call's work);
//                  this rank pushes no byte of call k into s's rx, ring or LL
//                  zone before it reads posted[s] >= k.  That is MPI's
//                  matched-receive order (mpi_perf.c:75,79,100,104,137,141):
//                  a payload of call k lands only under a receive of call k.
struct Mailbox {
    u64 flag[MPX_MAX_RANKS][kMaxPushWG];
    u64 ll[MPX_MAX_RANKS][kLLGranules];
    u64 credit[MPX_MAX_RANKS][kMaxPushWG];
    u64 posted[MPX_MAX_RANKS];
    u64 ready[MPX_MAX_RANKS];
};

// The end of a kernel-engine call: ONE 64-byte line of the host-mapped
// status, written by workgroup 0 with a single eight-lane store once every
// other store of the call has drained (Loop::finish_last).  The host spins on
// `word` = (u32)token | seal << 32, where the seal hashes the other seven
// words with the token: a line that became visible piecemeal does not match
// and is read again.  No drain sits between the line's fields and the word
// the host waits for — one PCIe write instead of a write, an
// acknowledgement and another write at the end of every call.
struct alignas(64) Fin {
    u64 recv_done;          // receives completed
    u64 recv_digest;        // check mode: sum of their finished checksums
    // phases (s_memrealtime, 100 MHz ticks), stamped by workgroup 0:
    u64 t_entry;            // started (after the go of an armed call)
    u64 t_posted;           // this side may push: the peer's receives are
                            // posted (0: this side pushes only after a receive)
    u64 t_first;            // the loop's first iteration done
    u64 t_loop;             // left the loop
    u64 t_exit;             // the call's end (every workgroup done)
    u64 word;               // fin_word(...): the host's completion word
};
__host__ __device__ inline u64 fin_mix(u64 z) {
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
__host__ __device__ inline u64 fin_word(u64 token, u64 v0, u64 v1, u64 v2, u64 v3, u64 v4, u64 v5, u64 v6) {
    u64 h = fin_mix(token ^ 0x6a09e667f3bcc909ull);
    h = fin_mix(h ^ v0);
    h = fin_mix(h ^ v1);
    h = fin_mix(h ^ v2);
    h = fin_mix(h ^ v3);
    h = fin_mix(h ^ v4);
    h = fin_mix(h ^ v5);
    h = fin_mix(h ^ v6);
    return (token & 0xffffffffull) | (h << 32);
}

// Per-rank host-mapped status words (written by the device, read by the host
// after the stream drains, or — the kernel engine — once `fin` is sealed).
struct Status {
    unsigned int err;       // bit0: a wait timed out
    unsigned int where;     // 1 + iteration index of the first timeout
    u64 spins;              // diagnostics: polls of the last wait
    // receive accounting of the last call, counted on the device where the
    // reference's call returns a receive (Recv, or Waitall for the
    // non-blocking loop, mpi_perf.c:75,79,110-111,122-123,137,141)
    u64 recv_done;          // receives completed (stream engines; the kernel
    u64 recv_digest;        // engine's are in fin) / check mode digest
    u64 seen, want;         // stream engines: flag value seen / awaited by the
                            // wait that timed out (diagnostics)
    u64 go;                 // armed call (mpx_xfer_arm): the host stores the
                            // call's token here to start it, token | kGoCancel
                            // to end it without a transfer
    u64 ready;              // armed call: its token once every workgroup is
                            // resident and waiting for go
    Fin fin;                // kernel engine: the end of the last call
};
constexpr u64 kGoCancel = 1ull << 63;

// Device scratch words of a rank ([0..3]: zero when a kernel-engine call
// starts — zeroed at attach, and reset by the last workgroup of every call, so
// no memset precedes the launch):
//   [0] grid-barrier counter  [1] abort word  [2] finished workgroups
//   [3] pull mode: chunks landed in rx this call (all receives, all workgroups)
//   [4..5] SDMA engine's device-side sequence base {tx, rx}
//   [6..7] RCCL engine's one-byte link set-up exchange
//   [8] armed call: workgroup 0's go verdict for the others (1 go, 2 cancel),
//       reset with [0..3]
//   [9] armed call: workgroups other than 0 waiting for go, reset with [0..3]
//   [10] host link: receives of this call workgroup 0 has seen arrive in host
//        memory, republished for the other workgroups; reset by the call's end
//   [11] host link: 1 once workgroup 0 has seen the endpoint's post; likewise
//   [12] full-duplex host link, check mode: the endpoint's credit word (the last
//        of this rank's pushes it has checked) as the pushing half's reader saw
//        it; in that call [10] holds the endpoint's ready word the same way;
//        both reset by the call's end
//   [13] full-duplex host link: chunks of this call's pushes drained (all
//        pushes, all pushing workgroups), as [3] counts the pulls; likewise
constexpr int kScratchWords = 16;
constexpr int kScrBar = 0, kScrAbort = 1, kScrFin = 2, kScrLanded = 3, kScrSeqBase = 4, kScrLink = 6, kScrGo = 8,
              kScrReady = 9, kScrHostSeen = 10, kScrHostPosted = 11, kScrHostCredit = 12, kScrHostSent = 13;

// Non-blocking check mode ("ring"): receive j of a call with `iters`
// iterations lands in slot (iters-1-j) mod S of the receiver, where slot 0 is
// rx itself (so rx ends holding the last payload, as in the reference) and
// slot s >= 1 is ring + (s-1)*B.  S = min(256, 1 + ring_bytes / B), computed
// from the RECEIVER's ring on both sides of the link.
inline int ring_slots(unsigned long long ring_bytes, long long len) {
    if (len <= 0) return kNbWindow;
    const unsigned long long s = 1 + ring_bytes / (unsigned long long)len;
    return s < (unsigned long long)kNbWindow ? (int)s : kNbWindow;
}
__host__ __device__ inline int ring_slot(int j, int iters, int slots) { return (iters - 1 - j) % slots; }

// A rank's latency recorder (mpx_lat_enable), in that rank's device memory.
// Written by lane 0 of workgroup 0 of the rank's traced calls (k_xfer_lat,
// k_xfer_pull_lat) — a rank runs one call at a time — and by the host only
// between calls, on the rank's stream (reset).  The block is allocated with
// room for raw_cap + 1 stamps behind it, and raw_cap stands in the block
// itself: the kernel bounds its raw stores by the very word the allocation
// was sized with.  The link recorder (mpx_fan_lat_enable) is nranks such
// blocks, one per peer rank, each written by lane 0 of that link's workgroup
// of the rank's traced LL fan calls (k_xfer_fan_ll<., true>; FanLLArgs.lat).
struct LatBlock {
    u64 count, calls, min_ticks, max_ticks, sum_ticks, max_iter, last_iters;   // mpx_lat's, accumulated
    u64 raw_cap;            // iterations of a call whose end stamp is kept (host, at enable)
    u64 raw_n;              // stamps of the last traced call in raw[]: 1 + min(iters, raw_cap)
    unsigned hist[MPX_LAT_BUCKETS];
    u64 raw[1];             // raw_cap + 1 stamps: t[0], then t[i+1] for i < raw_cap
};
inline size_t lat_block_bytes(int raw_cap) { return sizeof(LatBlock) + (size_t)raw_cap * sizeof(u64); }

// Arguments of one transfer loop on one rank (kernel engine).
struct XferArgs {
    const unsigned char* tx;     // local tx
    unsigned char* rx;           // local rx
    unsigned char* peer_rx;      // the peer's rx, mapped into this process
    Mailbox* my_mb;              // local mailbox (polled)
    Mailbox* peer_mb;            // peer's mailbox (written)
    Status* status;              // host-mapped
    u64* csum;                   // [iters] raw checksum sums (check mode)
    u64* gbar;                   // grid-barrier counter (check mode), zeroed
    u64 tx_seq0;                 // my last push seq on this link before the call
    u64 rx_seq0;                 // peer's last push seq on this link
    u64 timeout_ticks;           // s_memrealtime ticks (100 MHz) per wait
    long long len;               // B
    int iters;
    int mode;                    // enum mpx_mode
    int group;                   // 1 = sender side (group 1), 0 = group 0
    int my_slot;                 // my rank = my slot in the peer's mailbox
    int peer_slot;               // peer rank = its slot in my mailbox
    int nwg;                     // bulk push workgroups (same on both sides)
    int check;                   // 1 = checksum + poison each received payload
    int ll_max;                  // messages <= ll_max bytes use LL (<= kLLMaxBytes);
                                 // same on both sides of the link
    int stream;                  // 1: bulk payload stores add the nt hint (sc0 sc1 nt)
    int nb_publish;              // non-blocking mode: drain + flag every nb_publish
                                 // pushes (divides kNbWindow) and at the last
    int stage;                   // bytes of dynamic LDS holding this workgroup's
                                 // chunk of tx (0: bulk pushes read tx from HBM)
    // non-blocking check mode (k_xfer_nbcheck)
    unsigned char* ring;         // my receive slots 1..slots-1
    unsigned char* peer_ring;    // the peer's, mapped here
    u64* cnt;                    // [iters] workgroups done checking receive j
    int slots;                   // S: receive slots per link (ring_slots)
    int skip_push;               // test knob: 1 + iteration whose payload stores
                                 // are skipped (flag still published); 0 = off
    u64 call;                    // number of this call on the link (Mailbox.posted)
    int lag_wg;                  // test knob (MPX_TEST_LAG_WG): workgroup that stalls
    u64 lag_ticks;               //   lag_ticks before checking (non-blocking check
                                 //   mode) or pulling (pull mode) the call's last
                                 //   receive; 0 = off
    // pull mode (MPX_XFER_PULL, k_xfer_pull): bulk payloads are loaded by the
    // receiver from the sender's tx instead of stored by the sender
    const unsigned char* peer_tx;   // the peer's tx, mapped into this process
    int pull;                    // 1 = this call's bulk payloads are pulled
    int no_pull_wait;            // test knob (MPX_TEST_NO_PULL_WAIT): a sending side
                                 // ends without waiting for the peer's loads of tx
    u64 done_token;              // stored into Status.done by the last workgroup
    u64 go_token;                // armed call: wait for Status.go == go_token first
                                 // (0: start at once)
    u64 go_timeout_ticks;        // armed call: how long the kernel waits for go
    LatBlock* lat;               // the rank's latency recorder (mpx_lat_enable); null =
                                 // tracing off, and then no _lat kernel is launched
    // sequenced payloads (mpx_xfer_seq, k_xfer_seq): the pushing kernel generates
    // iteration i's payload from seq_tx_key ^ i << 24 instead of reading tx
    int seq;                     // 1 = launch_xfer picks the k_xfer_seq kernels
    u64 seq_tx_key;              // mpx_pattern_key(seed, my rank, peer rank, 0): this side's sends
    u64 seq_rx_key;              // mpx_pattern_key(seed, peer rank, my rank, 0): its receives (the
                                 // host's expectations; no kernel compares payloads itself)
};

// LL threshold of a link.  Within one GPU the bulk path's extra hop (payload
// drain, then flag) is cheap and bulk wins above ~2 KiB (loopback sweep,
// profiles/r01_loopback_sweep.jsonl; on the final LL path ping-pong from
// 3 KiB, r02_ll_threshold_ab.jsonl); across xGMI that hop is a full link
// round trip, so LL is kept up to its 8 KiB landing zone.
inline int ll_max_bytes(bool same_device) { return same_device ? 2048 : kLLMaxBytes; }

// LL granule tag for push sequence number `seq` (>= 1): never 0, so a zeroed
// mailbox can never match, and distinct for seqs < 2^31 apart.
__host__ __device__ inline unsigned ll_tag(u64 seq) {
    return (unsigned)(seq & 0x7fffffffull) | 0x80000000u;
}

// Workgroups of a bulk push of `len` bytes.  Both sides of a link evaluate
// this on the same inputs, so the receiver knows how many flags to expect.
constexpr long long kMinPushChunk = 1024;   // bytes per pushing workgroup, at least (link_nwg)
inline int bulk_nwg(long long len, bool same_device) {
    // ~32 KiB per workgroup across xGMI (enough 16-B stores in flight to
    // cover the link's bandwidth-delay product), 16 KiB within one GPU.
    const long long per = same_device ? (16 << 10) : (32 << 10);
    long long n = (len + per - 1) / per;
    // within one GPU both kernels of a pair, and of every other pair that
    // shares the GPU, must stay resident together: 128 keeps two pairs'
    // check-mode launches (4 x 128 workgroups) at half the chip's 4 per CU
    const long long cap = 128;
    if (n < 1) n = 1;
    if (n > cap) n = cap;
    return (int)n;
}
// The width of a link, pair or fan: the call's option, else the environment's
// value (MPX_PUSH_WG, MPX_FAN_WG), else the default rule's (bulk_nwg,
// fan_default_nwg); 0 if that exceeds kMaxPushWG (invalid).  A width chosen
// for large pushes is not applied to small ones: at least kMinPushChunk bytes
// per workgroup, and at least one workgroup (the size rule's chunks are
// 16-32 KiB, so it never narrows them).  Both sides of a link compute it from
// the same inputs, so they agree.
inline int link_nwg(int opt, int env, int dflt, long long len) {
    const int w = opt > 0 ? opt : env > 0 ? env : dflt;
    if (w > kMaxPushWG) return 0;
    const long long most = (len + kMinPushChunk - 1) / kMinPushChunk;
    const long long n = w < most ? w : most;
    return n < 1 ? 1 : (int)n;
}

// ---- fan exchange (mpx_xfer_fan, k_xfer_fan) --------------------------------
// One rank exchanges a block with each of several peers in ONE launch: the
// grid is the sum of the links' widths, and workgroup (k, w) pushes, receives
// and (check mode) checks chunk w of link k on its own.
//
// One record per link, in the rank's device memory, written by the host
// before the launch (on the rank's stream) and read back after it.
struct FanLink {
    unsigned char* peer_rx;   // where this rank's block lands: the peer's rx + my_rank * stride
    Mailbox* peer_mb;         // the peer's mailbox (written)
    u64 tx_seq0, rx_seq0;     // the link's push numbers before the call
    u64 call;                 // number of this call on the link (Mailbox.posted)
    long long off;            // peer * stride: the link's block in this rank's own tx and rx
    int peer;                 // the peer's rank = its slot in this rank's mailbox
    int nwg;                  // the link's width (the same on both sides)
    int csum0;                // k * iters: the link's first word of the checksum array
    int pad;
    // results, device atomics of the link's workgroups (host: ~0 and 0)
    u64 recv_done;            // min over the link's chunks of the receives completed
    u64 t_end;                // max over the link's workgroups of now_ticks() at their end
};
constexpr int kFanMaxGrid = 256;   // one rank's fan grid, at most (DESIGN.md "Fan exchange")
// the rank's fan table: the link records, then blockIdx.x -> link << 16 | w
struct FanTable {
    FanLink link[MPX_MAX_RANKS];
    unsigned map[kFanMaxGrid];
};
struct FanArgs {
    const unsigned char* tx;
    unsigned char* rx;
    Mailbox* my_mb;
    Status* status;
    u64* csum;                // [nlinks * iters] raw checksum sums (check mode)
    u64* gbar;                // the rank's scratch words
    FanTable* tab;
    u64 timeout_ticks;
    u64 done_token;
    long long len;            // block_len
    int iters, nlinks, my_slot;
    int check, stream, nb_publish, skip_push;
    // sequenced payloads (mpx_xfer_fan_seq): the pushes of link k generate iteration
    // i's block from mpx_pattern_key(seq_seed, my_slot, link k's peer, i) instead of
    // reading tx; the kernels derive the key, so FanLink stays as it is
    int seq;                  // 1 = launch_fan / launch_fan_ll pick the generating instantiations
    u64 seq_seed;
};

// The lock-step LL fan exchange (MPX_FAN_LL, k_xfer_fan_ll): one workgroup
// per link, the grid is nlinks (no workgroup map).  Push number s of a link
// lands in half s & 1 of the sender's LL row — kFanLLHalf granules each, so a
// block is at most MPX_FAN_LL_MAX bytes (DESIGN.md "Fan exchange").
constexpr int kFanLLHalf = kLLGranules / 2;
static_assert(kFanLLHalf * 4 == MPX_FAN_LL_MAX, "a half of the LL row holds one MPX_FAN_LL block");
struct FanLLArgs {
    FanArgs f;                // stream and nb_publish unused; check picks the instantiation
    int lag_link;             // test knob (MPX_TEST lag_wg): the link's workgroup that stalls
    u64 lag_ticks;            //   lag_ticks between its push and its wait of iteration iters / 2; 0 = off
    // the rank's link recorder (mpx_fan_lat_enable): nranks LatBlocks lat_stride
    // bytes apart (lat_block_bytes(raw_cap)), link k's at lat + peer * lat_stride —
    // keyed by the peer's rank, each written only by that link's workgroup.
    // null = tracing off, and then no _lat kernel is launched
    unsigned char* lat;
    u64 lat_stride;
};

// Default width of a fan link: the pair rule, capped so that the kernels of
// nranks ranks sharing one GPU (each up to nranks - 1 links wide) stay
// resident together.  Only things both ends of a link see alike go in.
inline int fan_default_nwg(long long block_len, bool same_device, int nranks) {
    const int share = nranks > 1 ? 128 / (nranks - 1) : 128;
    const int cap = share < 1 ? 1 : share;
    const int n = bulk_nwg(block_len, same_device);
    return n < cap ? n : cap;
}

// Fills the host image of a rank's fan table for a call whose links have the
// given widths: the records' widths and checksum offsets and the workgroup
// map, links interleaved over consecutive block indices (workgroup w of every
// link, then w + 1 of every link that wide).  Returns the grid, or -1 if it
// exceeds kFanMaxGrid or a width is out of range.  Pure host arithmetic
// (tools/fan_host_check.cpp runs it under the host sanitizers).
inline int fan_build_map(FanTable* tab, int nlinks, const int* nwg, int iters) {
    if (nlinks < 1 || nlinks > MPX_MAX_RANKS) return -1;
    long long grid = 0;
    int widest = 0;
    for (int k = 0; k < nlinks; ++k) {
        if (nwg[k] < 1 || nwg[k] > kMaxPushWG) return -1;
        grid += nwg[k];
        if (nwg[k] > widest) widest = nwg[k];
    }
    if (grid > kFanMaxGrid) return -1;
    int b = 0;
    for (int w = 0; w < widest; ++w)
        for (int k = 0; k < nlinks; ++k)
            if (w < nwg[k]) tab->map[b++] = ((unsigned)k << 16) | (unsigned)w;
    for (int k = 0; k < nlinks; ++k) {
        tab->link[k].nwg = nwg[k];
        tab->link[k].csum0 = k * iters;
    }
    return b;
}

// Launchers implemented in mpx_kernels.hip
hipError_t launch_fan(const FanArgs& a, int grid, hipStream_t s);
hipError_t launch_fan_ll(const FanLLArgs& a, hipStream_t s);   // grid = a.f.nlinks
hipError_t launch_xfer(const XferArgs& a, int grid, hipStream_t s);
// the host link's kernel (k_xfer_hostlink): ping-pong and unidir only; my_mb /
// peer_mb are the endpoint's out / in boxes, my_slot = peer_slot = this rank
hipError_t launch_hostlink(const XferArgs& a, int grid, hipStream_t s);
// the host link's full-duplex kernel (k_hostlink_duplex): the non-blocking
// loop on a split grid of 2 * a.nwg workgroups; the same boxes and slots
constexpr int kDuplexMaxWG = kMaxPushWG / 2;   // per direction
hipError_t launch_hostlink_duplex(const XferArgs& a, hipStream_t s);
// k_copy_win's resident window (DESIGN.md "k_copy tuning: the resident window").
// A copy is a row of 4 KiB blocks, one per workgroup.  Block b of src is
// loaded with the default cache policy, so that it stays in the 256 MiB
// Infinity Cache for the next copy of the same buffer, when
//     (b / unit) % period < window        (unit in blocks, period and window in units)
// and nontemporal otherwise (the stores: k_copy_win).  unit and period are powers of
// two: the kernel's test is a shift, a mask and a compare.  on = false is
// k_copy, the kernel without the choice.
struct CopyWindow {
    bool on = false;
    unsigned unit = 1, period = 1, window = 0;
};
constexpr size_t kCopyBlockBytes = 4096;
// The rule: a function of the copy's size alone, so repeated copies of the
// same pointers keep the same lines and no call needs to know of another.
// Constants from profiles/copy_window_lab.jsonl (1 GiB, form win_PL_*):
// stripes of 1 MiB units, 32 to a period, and as many units kept per period
// as hold kCopyWindowCap bytes resident over the whole copy.  Off below
// kCopyWindowMin (not landed below it: DESIGN.md) and where even one unit per
// period would pass the cap.
constexpr size_t kCopyWindowMin = (size_t)512 << 20;
constexpr size_t kCopyWindowCap = (size_t)192 << 20;
constexpr unsigned kCopyWindowUnit = 256, kCopyWindowPeriod = 32;
inline CopyWindow copy_window_rule(size_t n) {
    CopyWindow w;
    if (n < kCopyWindowMin) return w;
    const size_t period_bytes = (size_t)kCopyWindowUnit * kCopyWindowPeriod * kCopyBlockBytes;
    const size_t periods = (n + period_bytes - 1) / period_bytes;          // a partial last period counts as one
    const size_t units = kCopyWindowCap / ((size_t)kCopyWindowUnit * kCopyBlockBytes) / periods;
    if (!units) return w;
    w.on = true;
    w.unit = kCopyWindowUnit;
    w.period = kCopyWindowPeriod;
    w.window = units < kCopyWindowPeriod ? (unsigned)units : kCopyWindowPeriod;
    return w;
}
// MPX_COPY_WINDOW="period:window[:unit]" (read per call, like MPX_COPY; the
// tests and the A/B drive the kernel with it).  unit is in bytes (default
// 4096).  period and window are COUNTS OF UNITS written x 4096, as in the
// kernel's test above: the period in bytes is period / 4096 x unit, and the
// rule's choice at 1 GiB reads "131072:24576:1048576".  Every value is a
// multiple of 4096, unit / 4096 and period / 4096 are powers of two (the
// kernel shifts and masks), window <= period.  "0" is off: the kernel
// without the choice.  Returns false, with *w off, for anything else; *w is
// the rule's choice when v is null or empty.
inline bool copy_window_parse(const char* v, size_t n, CopyWindow* w) {
    *w = copy_window_rule(n);
    if (!v || !*v) return true;
    *w = CopyWindow();
    unsigned long long f[3] = {0, 0, kCopyBlockBytes};
    int k = 0;
    for (const char* p = v;; ++k) {
        if (k == 3 || *p < '0' || *p > '9') return false;
        unsigned long long x = 0;
        for (; *p >= '0' && *p <= '9'; ++p) {
            if (x > (1ull << 40)) return false;
            x = x * 10 + (unsigned long long)(*p - '0');
        }
        f[k] = x;
        if (!*p) break;
        if (*p++ != ':') return false;
    }
    if (k == 0) return f[0] == 0;
    const unsigned long long B = kCopyBlockBytes;
    if (f[0] % B || f[1] % B || f[2] % B || !f[0] || !f[2] || f[1] > f[0]) return false;
    const unsigned long long period = f[0] / B, unit = f[2] / B;
    if ((period & (period - 1)) || (unit & (unit - 1)) || period > (1u << 30) || unit > (1u << 30)) return false;
    w->on = true;
    w->unit = (unsigned)unit;
    w->period = (unsigned)period;
    w->window = (unsigned)(f[1] / B);
    return true;
}
hipError_t launch_copy(void* dst, const void* src, size_t n, hipStream_t s, int* grid_out,
                       const CopyWindow& win = CopyWindow());
// all `iters` copies in one launch with a grid barrier between steps; *bar
// must be 0 at launch
constexpr int kCopyStepsMaxGrid = 1024;   // 4 workgroups per CU: always co-resident
// copies up to 1 MiB run as k_copy_steps: faster than a launch per copy
// there (1 MiB 1.94-2.0 vs 2.4-2.7 us).  At 2 MiB one launch is faster in a
// fresh process (2.32-2.38 vs 2.42-2.94 us with 64 workgroups on one barrier
// counter, on three boxes) but bistable: after bench.py's headline and sweep
// it read 3.4-3.9 us on two boxes where a launch per copy read 2.6-3.0
// (profiles/r02_copy_steps_wgsize_mid.jsonl, r02_copy_sweep_state.jsonl), so
// the switch stays at 1 MiB; above it a launch per copy is as fast or faster
// (16 MiB 4.22 vs 5.15-5.95; r02_copy_steps_upl.jsonl, r02_copy_steps_mid.jsonl)
constexpr size_t kCopyStepsDefaultMax = (size_t)1 << 20;
// k_copy_pipe's range: (512 KiB, 16 MiB] (shape rule and numbers at
// launch_copy_pipe).  Per copy, in bench.py's sweep (right after the 1 GiB
// headline) and in fresh processes, against k_copy_steps / a launch per
// copy: 1 MiB 1.67-2.1 us (2.0 / 2.3-3.0), 4 MiB 2.56-2.59 (3.0 / 2.9-3.0),
// 8 MiB 3.2-3.9 (4.2 / 3.2-4.2), 16 MiB 4.3-6.0 (- / 5.0-6.8).  512 KiB:
// 1.56 vs the one-XCD steps form's 1.64 (kept).  16 MiB is the resident
// limit of 256 workgroups x 16 units per lane (r03_copy_pipe_ab.jsonl,
// r03_copy_pipe_state.jsonl, r03_copy_pipe_hier.jsonl).
constexpr size_t kCopyPipeDefaultMin = (size_t)512 << 10;
constexpr size_t kCopyPipeDefaultMax = (size_t)16 << 20;
hipError_t launch_copy_steps(void* dst, const void* src, size_t n, int iters, u64* bar, hipStream_t s,
                             int* grid_out, const int* shape = nullptr);
// all `iters` copies in one k_copy_pipe launch (copy s+1's loads in flight
// across copy s's grid barrier, a dedicated barrier wave); *bar must be 0
constexpr int kCopyPipeMaxGrid = 768;     // 320-lane workgroups, 3 per CU: resident
hipError_t launch_copy_pipe(void* dst, const void* src, size_t n, int iters, u64* bar, hipStream_t s,
                            int* grid_out, int upl_force = 0, int hier_force = -1);
hipError_t launch_fill(void* p, size_t n, int pattern, u64 arg, hipStream_t s);
hipError_t launch_checksum(const void* p, size_t n, u64* out_dev, hipStream_t s);
hipError_t launch_signal(u64* flag, const u64* base, u64 value, hipStream_t s);
hipError_t launch_wait(const u64* flag, const u64* base, u64 value, Status* st, u64 timeout_ticks, hipStream_t s);
hipError_t launch_seqbase(u64* base, u64 tx, u64 rx, int add, hipStream_t s);
// stream engines' receive accounting: st->recv_done += count and, when csum is
// set, st->recv_digest += sum_j (csum[j] ^ mix64(n)) over j in [j0, j0+count)
hipError_t launch_account(Status* st, const u64* csum, int j0, int count, long long n, hipStream_t s);

}  // namespace mpx
