// hostlink_lat_host_check — the CPU endpoint's latency recorder
// (mpi-perf_amd/csrc/mpx_hostlink.h: LatRec, run_loop<true>;
// include/mpx_hostlink_lat.h) as a stand-alone program for the host
// sanitizers: tools/asan_hostlink_lat.sh builds it with
// -fsanitize=address,undefined and once more with -fsanitize=thread and runs
// each once.  No GPU, no libmpx: a second CPU thread plays the kernel's side
// of the protocol on malloc'ed memory.  Covered: both modes and both
// orientations at 8 B, 256 B (LL), 257 B and 4161 B (bulk) with 0, 1, 7 and 33
// iterations and raw_cap 0, 4 and >= iters; two calls accumulating, then a
// reset; a host_lag at iteration 3 of 7; an untraced call between traced ones.
// Every block is recomputed from the raw deltas and compared field by field.
#include "mpx_hostlink.h"

#include <stdio.h>
#include <stdlib.h>

#include <thread>
#include <vector>

using namespace mpx::hostlink;

static int g_fail = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);      \
            ++g_fail;                                                       \
        }                                                                   \
    } while (0)

// ---- the kernel's side, on a CPU thread (no check mode, nothing lost) ----------
struct Gpu {
    HostMailbox* mb;
    const unsigned char* host_tx;
    unsigned char* host_rx;
    const unsigned char* tx;
    unsigned char* rx;
    int gpu, mode, group, iters;
    long long len;
    int nwg, ll_max;
    uint64_t seq0, call;
    int timed_out = 0;
};

static void chunk_of(long long n, int nwg, int w, long long* lo, long long* hi) {
    const long long chunk = (((n + nwg - 1) / nwg) + 15) & ~15ll;
    *lo = (long long)w * chunk;
    *hi = *lo + chunk < n ? *lo + chunk : n;
}

static void run_gpu(Gpu* g) {
    const detail::Waiter w{5.0};
    const bool unidir = g->mode == 2;
    const long long send_len = (unidir && g->group == 0) ? 1 : g->len;
    const long long recv_len = (unidir && g->group == 1) ? 1 : g->len;
    HostBox& in = g->mb->in;
    HostBox& out = g->mb->out;
    uint64_t txs = g->seq0, rxs = g->seq0;
    st_rel(&in.posted[g->gpu], g->call);
    if (g->iters > 0 && g->group == 1 && !w.until([&] { return ld_acq(&out.posted[g->gpu]) >= g->call; })) {
        g->timed_out = 1;
        return;
    }
    auto send = [&] {
        ++txs;
        if (send_len <= g->ll_max) {
            const uint64_t tag = (uint64_t)ll_tag(txs) << 32;
            for (int k = 0; k < 2 * ll_units(send_len); ++k) {
                uint32_t v = 0;
                const long long off = 4ll * k;
                if (off < send_len) memcpy(&v, g->tx + off, (size_t)(send_len - off < 4 ? send_len - off : 4));
                __atomic_store_n(&in.ll[g->gpu][k], tag | v, __ATOMIC_RELEASE);
            }
            return;
        }
        for (int k = 0; k < g->nwg; ++k) {
            long long lo, hi;
            chunk_of(send_len, g->nwg, k, &lo, &hi);
            if (lo < hi) memcpy(g->host_rx + lo, g->tx + lo, (size_t)(hi - lo));
            st_rel(&in.flag[g->gpu][k], txs);
        }
    };
    auto recv = [&] {
        ++rxs;
        if (recv_len <= g->ll_max) {
            const uint32_t tag = ll_tag(rxs);
            for (int k = 0; k < 2 * ll_units(recv_len); ++k) {
                uint64_t v = 0;
                if (!w.until([&] { return (uint32_t)((v = ld_acq(&out.ll[g->gpu][k])) >> 32) == tag; })) return false;
                const long long off = 4ll * k;
                const uint32_t d = (uint32_t)v;
                if (off < recv_len) memcpy(g->rx + off, &d, (size_t)(recv_len - off < 4 ? recv_len - off : 4));
            }
            return true;
        }
        if (!w.until([&] { return ld_acq(&out.ready[g->gpu]) >= rxs; })) return false;
        for (int k = 0; k < g->nwg; ++k) {
            long long lo, hi;
            chunk_of(recv_len, g->nwg, k, &lo, &hi);
            if (lo < hi) memcpy(g->rx + lo, g->host_tx + lo, (size_t)(hi - lo));
        }
        for (int k = 0; k < g->nwg; ++k) st_rel(&in.credit[g->gpu][k], rxs);
        return true;
    };
    for (int i = 0; i < g->iters; ++i) {
        if (g->group == 1) {
            send();
            if (!recv()) { g->timed_out = 1; return; }
        } else {
            if (!recv()) { g->timed_out = 1; return; }
            send();
        }
    }
}

// ---- a recorder block as mpx_hostlink_lat_enable allocates and clears it -------
struct Block {
    int cap;
    LatRec* b;
    explicit Block(int raw_cap) : cap(raw_cap), b(static_cast<LatRec*>(malloc(lat_rec_bytes(raw_cap)))) { reset(); }
    ~Block() { free(b); }
    Block(const Block&) = delete;
    void reset() {
        memset(b, 0, offsetof(LatRec, raw));
        b->raw_cap = (uint64_t)cap;
    }
    std::vector<unsigned char> bytes() const {
        const unsigned char* p = reinterpret_cast<const unsigned char*>(b);
        return std::vector<unsigned char>(p, p + lat_rec_bytes(cap));
    }
};

// what the block must hold after the traced calls whose raw deltas are `calls`
struct Want {
    uint64_t count = 0, calls = 0, mn = 0, mx = 0, sum = 0, maxi = 0, last = 0;
    uint32_t hist[MPX_LAT_BUCKETS] = {};
    void add(const std::vector<uint64_t>& t) {   // t[0 .. iters] of one call
        const uint64_t c0 = count;
        uint64_t cmn = ~0ull, cmx = 0, cmi = 0;
        for (size_t i = 0; i + 1 < t.size(); ++i) {
            const uint64_t d = t[i + 1] - t[i];
            if (d < cmn) cmn = d;
            if (d > cmx) { cmx = d; cmi = i; }
            ++hist[mpx_lat_bucket(d)];
            sum += d;
            ++count;
        }
        if (t.size() > 1) {
            if (c0 == 0 || cmn < mn) mn = cmn;
            if (c0 == 0 || cmx > mx) { mx = cmx; maxi = cmi; }
        }
        ++calls;
        last = t.size() - 1;
    }
    void check(const LatRec& b, int line) const {
        const bool same = b.count == count && b.calls == calls && b.last_iters == last && b.min_ticks == mn &&
                          b.max_ticks == mx && b.max_iter == maxi && b.sum_ticks == sum &&
                          memcmp(b.hist, hist, sizeof hist) == 0;
        if (!same) {
            fprintf(stderr, "line %d: block {count %llu calls %llu last %llu min %llu max %llu at %llu sum %llu} != "
                            "raw {%llu %llu %llu %llu %llu at %llu %llu}\n", line,
                    (unsigned long long)b.count, (unsigned long long)b.calls, (unsigned long long)b.last_iters,
                    (unsigned long long)b.min_ticks, (unsigned long long)b.max_ticks, (unsigned long long)b.max_iter,
                    (unsigned long long)b.sum_ticks, (unsigned long long)count, (unsigned long long)calls,
                    (unsigned long long)last, (unsigned long long)mn, (unsigned long long)mx, (unsigned long long)maxi,
                    (unsigned long long)sum);
            ++g_fail;
        }
    }
};

// ---- one link: an endpoint, the kernel's stand-in, their buffers and counters --
struct Link {
    size_t cap;
    HostMailbox* mb;
    std::vector<unsigned char> htx, hrx, gtx, grx;
    uint64_t seq = 0, calls = 0;
    explicit Link(size_t cap_) : cap(cap_), htx(cap_), hrx(cap_), gtx(cap_), grx(cap_) {
        mb = static_cast<HostMailbox*>(calloc(1, sizeof(HostMailbox)));
        uint64_t s = 0x13198a2e03707344ull;
        for (size_t k = 0; k < cap; ++k) {
            s = mix64(s + k);
            htx[k] = (unsigned char)s;
            gtx[k] = (unsigned char)(s >> 8);
        }
    }
    ~Link() { free(mb); }
    Link(const Link&) = delete;

    // One call, both sides at once; lat: the endpoint's block (nullptr: the
    // untraced entry point).  Returns the endpoint's stamps t[0 .. min(iters, raw_cap)].
    std::vector<uint64_t> call(int mode, int cpu_group, long long n, int iters, LatRec* lat, int lag_iter = -1,
                               long long lag_us = 0) {
        memset(hrx.data(), 0xEE, hrx.size());
        memset(grx.data(), 0xEE, grx.size());
        Call c;
        c.mb = mb;
        c.tx = htx.data();
        c.rx = hrx.data();
        c.gpu = 3;
        c.mode = mode;
        c.group = cpu_group;
        c.iters = iters;
        c.len = n;
        c.nwg = narrow_nwg(4, n);
        c.check = 1;
        c.expect = checksum(gtx.data(), (size_t)n);
        c.expect_ack = checksum(gtx.data(), 1);
        c.tx_seq0 = c.rx_seq0 = seq;
        if (iters > 0) ++calls;
        c.call = calls;
        c.timeout_s = 5.0;
        c.lag_iter = lag_iter;
        c.lag_us = lag_us;
        c.lat = lat;
        Gpu g{};
        g.mb = mb;
        g.host_tx = htx.data();
        g.host_rx = hrx.data();
        g.tx = gtx.data();
        g.rx = grx.data();
        g.gpu = 3;
        g.mode = mode;
        g.group = 1 - cpu_group;
        g.iters = iters;
        g.len = n;
        g.nwg = c.nwg;
        g.ll_max = c.ll_max;
        g.seq0 = seq;
        g.call = calls;
        Result r;
        std::thread th(run_gpu, &g);
        const int rc = lat ? run_loop<true>(c, &r) : run(c, &r);
        th.join();
        seq += (uint64_t)iters;
        const bool unidir = mode == 2;
        const long long cpu_recv = (unidir && cpu_group == 1) ? 1 : n;
        const long long gpu_recv = (unidir && cpu_group == 0) ? 1 : n;
        EXPECT(rc == 0 && !r.timed_out && !g.timed_out);
        EXPECT(r.recv_done == (uint64_t)iters && r.check_iters == (uint64_t)iters && r.check_failures == 0);
        if (iters > 0) {   // the bytes, as every case of this program verifies them
            EXPECT(memcmp(hrx.data(), gtx.data(), (size_t)cpu_recv) == 0);
            EXPECT(memcmp(grx.data(), htx.data(), (size_t)gpu_recv) == 0);
        }
        std::vector<uint64_t> t;
        if (lat) t.assign(lat->raw, lat->raw + lat->raw_n);
        return t;
    }
};

static void nondecreasing(const std::vector<uint64_t>& t) {
    for (size_t i = 0; i + 1 < t.size(); ++i) EXPECT(t[i] <= t[i + 1]);
}

int main() {
    const long long sizes[] = {8, 256, 257, 4161};
    const int iterss[] = {0, 1, 7, 33};
    Link l(8192);
    // every (mode, orientation, size, iterations) with raw_cap >= iters: the block against its own raw trace
    for (int mode : {0, 2})
        for (int cpu_group : {0, 1})
            for (long long n : sizes)
                for (int iters : iterss) {
                    Block b(40);
                    Want w;
                    const std::vector<uint64_t> t = l.call(mode, cpu_group, n, iters, b.b);
                    EXPECT(b.b->raw_n == 1 + (uint64_t)iters && t.size() == (size_t)iters + 1);
                    nondecreasing(t);
                    w.add(t);
                    w.check(*b.b, __LINE__);
                }
    // raw_cap 0 and 4: the raw trace is cut, the statistics cover every iteration
    for (int cap : {0, 4})
        for (int iters : iterss) {
            Block b(cap);
            const std::vector<uint64_t> t = l.call(0, iters & 1, 257, iters, b.b);
            const uint64_t kept = (uint64_t)(iters < cap ? iters : cap);
            EXPECT(b.b->raw_n == 1 + kept && t.size() == 1 + kept);
            nondecreasing(t);
            EXPECT(b.b->count == (uint64_t)iters && b.b->calls == 1 && b.b->last_iters == (uint64_t)iters);
            uint64_t in_hist = 0;
            for (int k = 0; k < MPX_LAT_BUCKETS; ++k) in_hist += b.b->hist[k];
            EXPECT(in_hist == (uint64_t)iters);
            if (iters > 0) EXPECT(b.b->min_ticks <= b.b->max_ticks && b.b->max_iter < (uint64_t)iters &&
                                  b.b->sum_ticks >= b.b->max_ticks && b.b->sum_ticks >= b.b->min_ticks * (uint64_t)iters);
            if (iters > 0 && kept == (uint64_t)iters) {
                Want w;
                w.add(t);
                w.check(*b.b, __LINE__);
            }
        }
    // two calls accumulate (an untraced call between them leaves the block byte-identical), then a reset
    {
        Block b(40);
        Want w;
        w.add(l.call(0, 1, 8, 7, b.b));
        w.check(*b.b, __LINE__);
        const std::vector<unsigned char> before = b.bytes();
        l.call(0, 1, 8, 5, nullptr);
        l.call(2, 0, 4161, 5, nullptr);
        EXPECT(before == b.bytes());
        w.add(l.call(2, 0, 4161, 33, b.b));
        w.check(*b.b, __LINE__);
        EXPECT(b.b->calls == 2 && b.b->count == 40 && b.b->last_iters == 33);
        w.add(l.call(0, 0, 256, 0, b.b));   // iters = 0: one more call, nothing else
        w.check(*b.b, __LINE__);
        EXPECT(b.b->calls == 3 && b.b->count == 40 && b.b->last_iters == 0 && b.b->raw_n == 1);
        b.reset();
        Want none;
        none.check(*b.b, __LINE__);
        EXPECT(b.b->raw_n == 0 && b.b->raw_cap == 40);
        Want again;
        again.add(l.call(0, 0, 257, 7, b.b));
        again.check(*b.b, __LINE__);
    }
    // host_lag at iteration 3 of 7: the lagged iteration is the maximum and at least the lag
    for (int mode : {0, 2})
        for (int cpu_group : {0, 1})
            for (long long n : {8ll, 4161ll}) {
                Block b(8);
                Want w;
                const long long lag_us = 20000;
                const std::vector<uint64_t> t = l.call(mode, cpu_group, n, 7, b.b, 3, lag_us);
                w.add(t);
                w.check(*b.b, __LINE__);
                EXPECT(b.b->max_iter == 3 && b.b->max_ticks >= (uint64_t)lag_us * 1000);
                // and the untraced entry point takes the knob too (it only waits)
                const double t0 = now_s();
                l.call(mode, cpu_group, n, 7, nullptr, 3, lag_us);
                EXPECT(now_s() - t0 >= lag_us * 1e-6);
            }
    // the clamp: 2^32 ns and more go into the last bucket (with [2^32 - 2^27, 2^32))
    EXPECT(mpx_lat_bucket((1ull << 32) - (1ull << 27) - 1) == MPX_LAT_BUCKETS - 2 &&
           mpx_lat_bucket(1ull << 32) == MPX_LAT_BUCKETS - 1 && mpx_lat_bucket(~0ull) == MPX_LAT_BUCKETS - 1);
    if (g_fail) {
        fprintf(stderr, "hostlink_lat_host_check: %d failures\n", g_fail);
        return 1;
    }
    puts("hostlink_lat_host_check: ok");
    return 0;
}
