// mpx_hostlink.h — the host link's shared memory layout and the CPU endpoint's
// side of the transfer loops (include/mpx_hostlink.h: mpx_host_xfer;
// include/mpx_hostlink_duplex.h: mpx_host_xfer_duplex).  Plain
// C++: no HIP include, every shared word is a uint64_t read and written
// through the __atomic_* builtins, so the file builds with g++ alone
// (tools/hostlink_host_check.cpp and tools/hostlink_duplex_host_check.cpp run
// it under the host sanitizers with a second CPU thread in the GPU's place).
//
// A host endpoint cannot write device memory, so every word and byte that
// crosses the link lives in pinned host memory and the GPU does all the
// moving (DESIGN.md §5 "Host link"):
//   GPU -> CPU  LL granules into in.ll, or a bulk push into the endpoint's rx
//               (payload stores, per-workgroup drain, then in.flag[w]);
//   CPU -> GPU  LL granules into out.ll, which the GPU's workgroup 0 polls
//               across the link, or "tx holds message k" in out.ready, after
//               which the GPU's workgroups load their chunks of the
//               endpoint's tx themselves and answer with in.credit[w].
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <time.h>

// mpx_lat_bucket and MPX_LAT_BUCKETS: one definition for host and device (plain C)
#include "../../include/mpx.h"
// the sequenced payloads' pattern and checksum (run_loop's SEQ form)
#include "mpx_seq.h"

#if defined(__x86_64__) || defined(__i386__)
#include <immintrin.h>
#endif

namespace mpx {
namespace hostlink {

// the library's limits (mpx_internal.h; mpx_engine_hostlink.hip asserts them equal)
constexpr int kRanks = 64;          // MPX_MAX_RANKS
constexpr int kWG = 256;            // kMaxPushWG: flag / credit words per link
constexpr int kLLBytes = 8192;      // kLLMaxBytes: the LL landing row
constexpr int kGranules = kLLBytes / 4;
constexpr int kMinChunk = 1024;     // kMinPushChunk
// The LL threshold: the largest size of the probe's sweep (256 B ... 8 KiB,
// powers of two) at which LL granules were not slower than the bulk form —
// across PCIe a granule poll is a link round trip, and from 512 B on the bulk
// form's one flag per workgroup wins (profiles/hostlink.jsonl)
constexpr int kDefaultLL = 256;
// The default width's cap: unidir at 4 MiB read best at 4-32 workgroups in
// both directions and lost 11-22 % at the pair rule's 128 (same profile)
constexpr int kDefaultMaxWG = 16;

// One direction of a host endpoint's mailbox.  It has the layout of the
// device mailbox (Mailbox, mpx_internal.h), so the kernels' pushes, polls and
// pulls address it as they address a GPU peer's.  Rows are indexed by the GPU
// peer's rank.
struct HostBox {
    uint64_t flag[kRanks][kWG];       // sequence number of the last bulk push of workgroup w
    uint64_t ll[kRanks][kGranules];   // LL granules {tag:32 | payload:32}
    uint64_t credit[kRanks][kWG];     // last pulled push whose chunk w is done with
    uint64_t posted[kRanks];          // "receives posted": the link's call number
    uint64_t ready[kRanks];           // "tx holds message k"
};
// in : written by the GPU, read by the CPU   — flag, ll, credit, posted
// out: written by the CPU, polled by the GPU — ll (the ll_out row), ready, posted,
//      and credit[gpu][0] (the full-duplex loop's check mode: the last of the
//      GPU's pushes the CPU has checked and poisoned)
struct HostMailbox {
    HostBox in;
    HostBox out;
};

inline void cpu_pause() {
#if defined(__x86_64__) || defined(__i386__)
    _mm_pause();
#endif
}
inline double now_s() {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + (double)ts.tv_nsec * 1e-9;
}
inline uint64_t now_ns() {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (uint64_t)ts.tv_sec * 1000000000ull + (uint64_t)ts.tv_nsec;
}
inline uint64_t ld_acq(const uint64_t* p) { return __atomic_load_n(p, __ATOMIC_ACQUIRE); }
inline void st_rel(uint64_t* p, uint64_t v) { __atomic_store_n(p, v, __ATOMIC_RELEASE); }

inline uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
// mpx_checksum's value (oracle_checksum): the sum over the
// zero-padded little-endian 64-bit words w_k of mix64(w_k + (k + 1) * golden),
// finished with ^ mix64(n).  Any alignment.
inline uint64_t checksum(const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    uint64_t sum = 0;
    size_t k = 0;
    for (; 8 * k + 8 <= n; ++k) {
        uint64_t w;
        memcpy(&w, b + 8 * k, 8);
        sum += mix64(w + (k + 1) * 0x9E3779B97F4A7C15ull);
    }
    if (8 * k < n) {
        uint64_t w = 0;
        memcpy(&w, b + 8 * k, n - 8 * k);
        sum += mix64(w + (k + 1) * 0x9E3779B97F4A7C15ull);
    }
    return sum ^ mix64((uint64_t)n);
}
// The kernels' poison of iteration `iter`, form by form (Loop::check): an LL
// message gets the pattern's low byte in every byte; a bulk message the 64-bit
// pattern over its whole 16-byte units (Loop::sum_chunk: chunks are multiples
// of 16 bytes, so the units are the message's) and the low byte over the
// tail.  Any value that differs from the payload would serve; it is the same
// one so that a poisoned rx reads alike whichever side received.
inline void poison(unsigned char* p, size_t n, int iter, bool ll) {
    const uint64_t w = 0x5a5a5a5a5a5a5a5aull ^ (uint64_t)iter;
    const size_t units = ll ? 0 : n & ~(size_t)15;   // bytes in whole 16-byte units
    for (size_t o = 0; o < units; o += 8) memcpy(p + o, &w, 8);
    for (size_t o = units; o < n; ++o) p[o] = (unsigned char)w;
}

// ll_tag (mpx_internal.h): never 0, distinct for push numbers < 2^31 apart
inline uint32_t ll_tag(uint64_t seq) { return (uint32_t)(seq & 0x7fffffffull) | 0x80000000u; }
// 16-byte units of an LL message: the kernels store and poll whole units, so
// both granules of the last unit carry the tag; a 0-byte message is one unit
inline int ll_units(long long n) {
    const int ng = n > 0 ? (int)((n + 3) >> 2) : 1;
    return (ng + 1) >> 1;
}
// link_nwg's narrowing (mpx_internal.h): at least kMinChunk bytes per workgroup
inline int narrow_nwg(int w, long long len) {
    const long long most = (len + kMinChunk - 1) / kMinChunk;
    const long long n = w < most ? w : most;
    return n < 1 ? 1 : (int)n;
}

// An endpoint's latency recorder block (include/mpx_hostlink_lat.h), in
// ordinary host memory: mpx_lat's accumulated fields, the raw_cap in force
// and the last traced call's stamps, in CLOCK_MONOTONIC nanoseconds.  It has
// the device block's layout (LatBlock, mpx_internal.h) and is allocated with
// room for raw_cap + 1 stamps.  Written by the thread inside run_traced() and
// by the caller only between that endpoint's calls.
struct LatRec {
    uint64_t count, calls, min_ticks, max_ticks, sum_ticks, max_iter, last_iters;
    uint64_t raw_cap;          // iterations of a call whose end stamp is kept
    uint64_t raw_n;            // stamps of the last traced call in raw[]: 1 + min(iters, raw_cap)
    uint32_t hist[MPX_LAT_BUCKETS];
    uint64_t raw[1];           // raw_cap + 1 stamps: t[0], then t[i+1] for i < raw_cap
};
inline size_t lat_rec_bytes(int raw_cap) { return sizeof(LatRec) + (size_t)raw_cap * sizeof(uint64_t); }

// One call of the CPU endpoint.
struct Call {
    HostMailbox* mb = nullptr;
    const unsigned char* tx = nullptr;
    unsigned char* rx = nullptr;
    int gpu = 0;               // the GPU peer's rank: the mailbox row
    int mode = 0, group = 0;   // enum mpx_mode (0 ping-pong, 2 unidir); 1 = sends first
    int iters = 0;
    long long len = 0;
    int nwg = 1;               // the link's width (both ends compute it alike)
    int ll_max = kDefaultLL;   // messages <= ll_max go as LL granules
    int check = 0;
    uint64_t expect = 0, expect_ack = 0;
    uint64_t tx_seq0 = 0, rx_seq0 = 0;   // the link's push numbers before the call
    uint64_t call = 0;         // the link's call number (posted)
    double timeout_s = 10.0;   // per wait, CLOCK_MONOTONIC
    int skip_push = 0;         // test knob: 1 + the iteration whose payload is lost
    int lag_iter = -1;         // test knob (host_lag): the iteration before whose first step
    long long lag_us = 0;      //   the endpoint busy-waits lag_us; -1 = off
    LatRec* lat = nullptr;     // the block of the GPU peer (run_traced); nullptr = untraced
    // a sequenced call (run_seq; include/mpx_hostlink_seq.h)
    unsigned char* seq_tx = nullptr;        // the endpoint's tx, writable: a bulk send's payload is written here
    uint64_t seq_tx_key = 0;                // seq::key_base(seed, endpoint, gpu): this side's sends
    const uint64_t* expect_each = nullptr;  // check: [iters] checksums of the payloads this side receives
    int seq_stale = 0;         // test knob: 1 + the iteration whose send repeats the payload before it
};
struct Result {
    uint64_t recv_done = 0, recv_digest = 0, check_iters = 0;
    int check_failures = 0;
    int timed_out = 0;         // 1: a wait ran past its deadline,
    int where = 0;             //    at this iteration
};

namespace detail {

struct Waiter {
    double timeout_s;
    // spins until pred() holds; false once the deadline has passed
    template <class Pred>
    bool until(Pred pred) const {
        const double t0 = now_s();
        for (unsigned spins = 1;; ++spins) {
            if (pred()) return true;
            if ((spins & 255) == 0 && now_s() - t0 > timeout_s) return pred();
            cpu_pause();
        }
    }
};

// CPU -> GPU, LL: granules into out.ll; data and tag share their 8 bytes, so
// each granule is one store and the GPU's poll that sees the tag holds the data
inline void send_ll(const Call& c, long long n, uint64_t seq, bool lose) {
    uint64_t* row = c.mb->out.ll[c.gpu];
    const uint64_t tag = (uint64_t)ll_tag(seq) << 32;
    const int ng = 2 * ll_units(n);
    for (int g = 0; g < ng; ++g) {
        uint32_t w = 0;
        const long long off = 4ll * g;
        if (!lose && off < n) memcpy(&w, c.tx + off, (size_t)(n - off < 4 ? n - off : 4));
        __atomic_store_n(&row[g], tag | w, __ATOMIC_RELEASE);
    }
}
// CPU -> GPU, LL, sequenced: the same granules packed from the generated words
// of the pattern `key`; tx is not touched
inline void send_ll_gen(const Call& c, long long n, uint64_t push, uint64_t key, bool lose) {
    uint64_t* row = c.mb->out.ll[c.gpu];
    const uint64_t tag = (uint64_t)ll_tag(push) << 32;
    const int ng = 2 * ll_units(n);
    for (int g = 0; g < ng; ++g) {
        uint32_t w = 0;
        const long long off = 4ll * g;
        if (!lose && off < n) {
            w = (uint32_t)(seq::fill_word(key, (uint64_t)(g >> 1)) >> (32 * (g & 1)));
            if (n - off < 4) w &= (1u << (8 * (int)(n - off))) - 1;
        }
        __atomic_store_n(&row[g], tag | w, __ATOMIC_RELEASE);
    }
}
// GPU -> CPU, LL: every granule's tag, then the unpack into rx[0:n)
inline bool recv_ll(const Call& c, const Waiter& w, long long n, uint64_t seq) {
    const uint64_t* row = c.mb->in.ll[c.gpu];
    const uint32_t tag = ll_tag(seq);
    const int ng = 2 * ll_units(n);
    for (int g = 0; g < ng; ++g) {
        uint64_t v = 0;
        if (!w.until([&] { return (uint32_t)((v = ld_acq(&row[g])) >> 32) == tag; })) return false;
        const long long off = 4ll * g;
        if (off < n) {
            const uint32_t d = (uint32_t)v;
            memcpy(c.rx + off, &d, (size_t)(n - off < 4 ? n - off : 4));
        }
    }
    return true;
}
// GPU -> CPU, bulk: the GPU's workgroups stored their chunks into rx and
// drained before their flags
inline bool recv_bulk(const Call& c, const Waiter& w, uint64_t seq) {
    const uint64_t* f = c.mb->in.flag[c.gpu];
    for (int k = 0; k < c.nwg; ++k)
        if (!w.until([&] { return ld_acq(&f[k]) >= seq; })) return false;
    return true;
}
// CPU -> GPU, bulk: tx holds the message; the GPU pulls it and credits every chunk
inline bool send_bulk(const Call& c, const Waiter& w, uint64_t seq) {
    st_rel(&c.mb->out.ready[c.gpu], seq);
    const uint64_t* cr = c.mb->in.credit[c.gpu];
    for (int k = 0; k < c.nwg; ++k)
        if (!w.until([&] { return ld_acq(&cr[k]) >= seq; })) return false;
    return true;
}

// The endpoint's per-iteration stamps, as the kernels' LatTrace takes them: the
// deltas stream into locals (min, max, the iteration of the first maximum; the
// sum telescopes), one add on the histogram bucket and, while i < raw_cap, one
// store of the stamp; the fold into the block comes after the loop.
// Trace<false> is empty: the untraced loop reads no clock for it.
template <bool LAT>
struct Trace {
    void begin(LatRec*, int) {}
    void tick(int) {}
    void end() {}
};
template <>
struct Trace<true> {
    LatRec* blk = nullptr;
    uint64_t prev = 0, mn = ~0ull, mx = 0;
    uint64_t cap = 0, maxi = 0, n = 0;
    void begin(LatRec* b, int iters) {
        blk = b;
        cap = (uint64_t)iters < b->raw_cap ? (uint64_t)iters : b->raw_cap;
        prev = now_ns();
        b->raw[0] = prev;
    }
    void tick(int i) {
        const uint64_t t = now_ns();
        const uint64_t d = t - prev;
        prev = t;
        if (d < mn) mn = d;
        if (d > mx) {
            mx = d;
            maxi = (uint64_t)i;
        }
        ++n;
        ++blk->hist[mpx_lat_bucket(d)];   // (2^32 ns and more: the last bucket)
        if ((uint64_t)i < cap) blk->raw[i + 1] = t;
    }
    void end() {
        LatRec& b = *blk;
        if (n) {
            if (b.count == 0 || mn < b.min_ticks) b.min_ticks = mn;
            if (b.count == 0 || mx > b.max_ticks) {
                b.max_ticks = mx;
                b.max_iter = maxi;
            }
            b.sum_ticks += prev - b.raw[0];
            b.count += n;
        }
        b.calls += 1;
        b.last_iters = n;
        b.raw_n = 1 + (n < cap ? n : cap);
    }
};

}  // namespace detail

// The endpoint's side of the reference's ping-pong (mpi_perf.c:66-83) or
// unidirectional (:127-145) loop on the calling thread.  Returns 0, or 1 after
// a wait that ran out (r->timed_out, r->where).
//   LAT: the traced form (c.lat, include/mpx_hostlink_lat.h).  t[0] is taken
// right before the loop — out.posted is stored and, on a side that sends
// first, the peer's post was seen — and t[i+1] when iteration i's last step
// has returned, check and poison included: one clock_gettime per iteration.
// A call that times out leaves the block as the loop left it (undefined until
// reset).  LAT = false reads the clock only where its waits always did.
//   SEQ: a sequenced call (run_seq).  Send i carries P(seed, endpoint, gpu, i,
// send_len), the pattern of seq::key_of(c.seq_tx_key, i): an LL send packs its
// granules from the generated words, a bulk send writes the pattern into
// c.seq_tx[0 : send_len) and then says "tx holds message k" as ever.  That
// write is the one thing the ordinary loop never does, and what makes it safe
// is the loop's own order: send_bulk returns only after every chunk's credit,
// so when send i + 1 writes tx every load of send i has been answered.  This
// is the invariant a sequenced call puts under test — a credit taken early, or
// a pull served from a stale copy, now costs bytes the GPU's check can see.
// Receive i is compared with c.expect_each[i].
template <bool LAT, bool SEQ = false>
inline int run_loop(const Call& c, Result* r) {
    using namespace detail;
    *r = Result{};
    const Waiter w{c.timeout_s};
    const bool unidir = c.mode == 2;
    const long long send_len = (unidir && c.group == 0) ? 1 : c.len;
    const long long recv_len = (unidir && c.group == 1) ? 1 : c.len;
    const uint64_t want = (unidir && c.group == 1) ? c.expect_ack : c.expect;
    uint64_t txs = c.tx_seq0, rxs = c.rx_seq0;
    // this call's receives are posted; a side that sends first waits for the peer's
    st_rel(&c.mb->out.posted[c.gpu], c.call);
    if (c.iters > 0 && c.group == 1 && !w.until([&] { return ld_acq(&c.mb->in.posted[c.gpu]) >= c.call; })) {
        r->timed_out = 1;
        return 1;
    }
    auto send = [&](int i) {
        ++txs;
        if constexpr (SEQ) {
            const bool lose = !(unidir && c.group == 0) && c.skip_push == i + 1;
            // test knob (seq_stale): this send repeats the payload before it —
            // an LL send packs key i - 1, a bulk send leaves tx as it is; the
            // first send of a call has no predecessor and sends what tx held
            const bool stale = c.seq_stale == i + 1;
            if (send_len <= c.ll_max) {
                if (stale && i == 0) send_ll(c, send_len, txs, lose);
                else send_ll_gen(c, send_len, txs, seq::key_of(c.seq_tx_key, stale ? i - 1 : i), lose);
                return true;
            }
            // strictly after the credits of send i - 1 (above): tx is quiet
            if (!stale) seq::pattern(c.seq_tx, (size_t)send_len, seq::key_of(c.seq_tx_key, i));
            return send_bulk(c, w, txs);
        }
        if (send_len <= c.ll_max) {
            send_ll(c, send_len, txs, !(unidir && c.group == 0) && c.skip_push == i + 1);   // (never an ack)
            return true;
        }
        return send_bulk(c, w, txs);   // (a lost bulk payload is the puller's to lose)
    };
    auto recv = [&](int i) {
        ++rxs;
        if (!(recv_len <= c.ll_max ? recv_ll(c, w, recv_len, rxs) : recv_bulk(c, w, rxs))) return false;
        ++r->recv_done;
        if (c.check) {
            const uint64_t got = checksum(c.rx, (size_t)recv_len);
            r->recv_digest += got;
            ++r->check_iters;
            if (got != (SEQ ? c.expect_each[i] : want)) ++r->check_failures;
            if (i + 1 != c.iters) poison(c.rx, (size_t)recv_len, i, recv_len <= c.ll_max);   // the last payload stays
        }
        return true;
    };
    Trace<LAT> T;
    if (LAT) T.begin(c.lat, c.iters);
    for (int i = 0; i < c.iters; ++i) {
        if (i == c.lag_iter && c.lag_us > 0) {   // test knob (host_lag)
            const double t0 = now_s();
            while ((now_s() - t0) * 1e6 < (double)c.lag_us) cpu_pause();
        }
        const bool ok = c.group == 1 ? (send(i) && recv(i)) : (recv(i) && send(i));
        if (!ok) {
            r->timed_out = 1;
            r->where = i;
            return 1;
        }
        if (LAT) T.tick(i);
    }
    if (LAT) T.end();
    return 0;
}
// the untraced entry point (mpx_host_xfer calls run_loop<true> when c.lat is set)
inline int run(const Call& c, Result* r) { return run_loop<false>(c, r); }
// a sequenced call's (mpx_host_xfer_seq): never traced, c.lat is not read
inline int run_seq(const Call& c, Result* r) { return run_loop<false, true>(c, r); }

// The endpoint's side of the reference's non-blocking loop (mpi_perf.c:85-125)
// on the calling thread — the full-duplex loop of include/mpx_hostlink_duplex.h;
// c.mode and c.group are not read (both sides run the same loop), nor is
// c.ll_max (there is no LL form) or c.skip_push (the GPU loses both
// directions' payloads: it does all the moving).
//   Isend i   one release store of out.ready = tx_seq0 + i + 1: tx holds the
//             message, the GPU's pulling workgroups load it and answer with
//             in.credit[w] (on their publish schedule);
//   Irecv i   rx itself: the GPU's pushing workgroups store their chunks and
//             publish in.flag[w] (on theirs);
//   Waitall   at window slot 255 over the sends and receives of slots 0..254,
//             and over what is in flight after the loop; slot 255 of each
//             full window is never waited for, so recv_done = iters - iters / 256.
// The call returns only once every one of its sends was pulled (every credit)
// and every payload is in (every flag): rx and tx are quiet then.
//   Check mode: every payload is checksummed in order as it lands, the
// uncounted ones too; every one but the last is poisoned, and then out.credit
// [gpu][0] says so — the GPU stores push i + 1 only after that (a one-slot
// ring: all receives share rx).  Every wait services landed receives while it
// waits, so neither side starves the other; a serviced receive restarts the
// wait's deadline.
// Returns 0, or 1 after a wait that ran out (r->timed_out, r->where).
inline int run_duplex(const Call& c, Result* r) {
    using namespace detail;
    *r = Result{};
    const uint64_t* flag = c.mb->in.flag[c.gpu];
    const uint64_t* credit = c.mb->in.credit[c.gpu];
    int next = 0;   // check mode: the next receive to check
    auto landed = [&](uint64_t seq) {
        for (int k = 0; k < c.nwg; ++k)
            if (ld_acq(&flag[k]) < seq) return false;
        return true;
    };
    auto pulled = [&](uint64_t seq) {
        for (int k = 0; k < c.nwg; ++k)
            if (ld_acq(&credit[k]) < seq) return false;
        return true;
    };
    auto service = [&]() {
        bool any = false;
        while (c.check && next < c.iters && landed(c.rx_seq0 + (uint64_t)next + 1)) {
            const uint64_t got = checksum(c.rx, (size_t)c.len);
            if (next % 256 != 255) r->recv_digest += got;   // the counted receives
            ++r->check_iters;
            if (got != c.expect) ++r->check_failures;
            if (next + 1 != c.iters) poison(c.rx, (size_t)c.len, next, false);   // the last payload stays
            st_rel(&c.mb->out.credit[c.gpu][0], c.rx_seq0 + (uint64_t)next + 1);
            ++next;
            any = true;
        }
        return any;
    };
    // Waitall over the first `upto` sends and receives of the call
    auto waitall = [&](int upto) {
        const uint64_t txs = c.tx_seq0 + (uint64_t)upto, rxs = c.rx_seq0 + (uint64_t)upto;
        auto done = [&] { return pulled(txs) && (c.check ? next >= upto : landed(rxs)); };
        double t0 = now_s();
        for (unsigned spins = 1;; ++spins) {
            if (service()) t0 = now_s();
            if (done()) return true;
            if ((spins & 255) == 0 && now_s() - t0 > c.timeout_s) return done();
            cpu_pause();
        }
    };
    // this call's receives are posted; nothing is pushed from here (the GPU
    // pulls this side's sends, and only inside its own call), so the peer's
    // post is not waited for
    st_rel(&c.mb->out.posted[c.gpu], c.call);
    int inflight = 0;
    for (int i = 0; i < c.iters; ++i) {
        st_rel(&c.mb->out.ready[c.gpu], c.tx_seq0 + (uint64_t)i + 1);   // Isend; the Irecv is rx
        service();
        if (inflight == 255) {                          // Waitall(255): iterations i-255 .. i-1
            if (!waitall(i)) {
                r->timed_out = 1;
                r->where = i;
                return 1;
            }
            r->recv_done += (uint64_t)inflight;
            inflight = 0;
        } else {
            ++inflight;
        }
    }
    // Waitall(inflight) — and the pending slot 255 of a last full window too:
    // counted it is not, but its send must be complete and its payload in
    if (c.iters > 0 && !waitall(c.iters)) {
        r->timed_out = 1;
        r->where = c.iters - 1;
        return 1;
    }
    r->recv_done += (uint64_t)inflight;
    return 0;
}

}  // namespace hostlink
}  // namespace mpx
