// hostlink_host_check — the CPU endpoint of the host link
// (mpi-perf_amd/csrc/mpx_hostlink.h) as a stand-alone program for the host
// sanitizers: tools/asan_hostlink.sh builds it with
// -fsanitize=address,undefined and once more with -fsanitize=thread and runs
// each once.  No GPU, no libmpx: a second CPU thread plays the GPU's side of
// the same protocol (what k_xfer_hostlink does with its pushes, polls, pulls
// and credits) on malloc'ed memory.  Covered: both modes, both orientations,
// sizes on both sides of the LL threshold, check mode, several calls on one
// link, links that start just short of push 2^31, push 2^32 and call 2^32, a
// lost payload in each direction and form, and a peer that never comes (the
// CPU's deadline).
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

// ---- the GPU's side, on a CPU thread ----------------------------------------
struct Gpu {
    HostMailbox* mb;
    const unsigned char* host_tx;   // the endpoint's buffers, as the kernel maps them
    unsigned char* host_rx;
    const unsigned char* tx;        // the GPU rank's own
    unsigned char* rx;
    int gpu, mode, group, iters;
    long long len;
    int nwg, ll_max, check;
    uint64_t expect, expect_ack, tx_seq0, rx_seq0, call;
    int lose_push = 0, lose_pull = 0;   // 1 + the iteration whose payload this side loses
    uint64_t recv_done = 0, digest = 0;
    int failures = 0, timed_out = 0;
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
    const uint64_t want = (unidir && g->group == 1) ? g->expect_ack : g->expect;
    HostBox& in = g->mb->in;
    HostBox& out = g->mb->out;
    uint64_t txs = g->tx_seq0, rxs = g->rx_seq0;
    st_rel(&in.posted[g->gpu], g->call);
    if (g->iters > 0 && g->group == 1 && !w.until([&] { return ld_acq(&out.posted[g->gpu]) >= g->call; })) {
        g->timed_out = 1;
        return;
    }
    auto send = [&](int i) {
        ++txs;
        const bool lose = !(unidir && g->group == 0) && g->lose_push == i + 1;
        if (send_len <= g->ll_max) {
            const uint64_t tag = (uint64_t)ll_tag(txs) << 32;
            for (int k = 0; k < 2 * ll_units(send_len); ++k) {
                uint32_t v = lose ? ~0u : 0;
                const long long off = 4ll * k;
                if (!lose && off < send_len) memcpy(&v, g->tx + off, (size_t)(send_len - off < 4 ? send_len - off : 4));
                __atomic_store_n(&in.ll[g->gpu][k], tag | v, __ATOMIC_RELEASE);
            }
            return;
        }
        for (int k = 0; k < g->nwg; ++k) {
            long long lo, hi;
            chunk_of(send_len, g->nwg, k, &lo, &hi);
            if (lo < hi && !lose) memcpy(g->host_rx + lo, g->tx + lo, (size_t)(hi - lo));
            st_rel(&in.flag[g->gpu][k], txs);
        }
    };
    auto recv = [&](int i) {
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
        } else {
            if (!w.until([&] { return ld_acq(&out.ready[g->gpu]) >= rxs; })) return false;
            for (int k = 0; k < g->nwg; ++k) {
                long long lo, hi;
                chunk_of(recv_len, g->nwg, k, &lo, &hi);
                if (lo < hi && g->lose_pull != i + 1) memcpy(g->rx + lo, g->host_tx + lo, (size_t)(hi - lo));
            }
            // (the kernel checks its chunk before it credits it; the order does not matter here:
            // the endpoint's tx does not change while the loop runs)
            for (int k = 0; k < g->nwg; ++k) st_rel(&in.credit[g->gpu][k], rxs);
        }
        ++g->recv_done;
        if (g->check) {
            const uint64_t got = checksum(g->rx, (size_t)recv_len);
            g->digest += got;
            if (got != want) ++g->failures;
            if (i + 1 != g->iters) poison(g->rx, (size_t)recv_len, i, recv_len <= g->ll_max);
        }
        return true;
    };
    for (int i = 0; i < g->iters; ++i) {
        if (g->group == 1) {
            send(i);
            if (!recv(i)) { g->timed_out = 1; return; }
        } else {
            if (!recv(i)) { g->timed_out = 1; return; }
            send(i);
        }
    }
}

// ---- one link: an endpoint, a GPU rank, their buffers and counters ------------
struct Link {
    static constexpr size_t kGuard = 64;
    size_t cap;
    HostMailbox* mb;
    std::vector<unsigned char> htx, hrx, gtx, grx;
    uint64_t seq = 0, calls = 0;
    int ll_max = kDefaultLL;
    explicit Link(size_t cap_) : cap(cap_), htx(cap_ + kGuard), hrx(cap_ + kGuard), gtx(cap_ + kGuard), grx(cap_ + kGuard) {
        mb = static_cast<HostMailbox*>(calloc(1, sizeof(HostMailbox)));
        uint64_t s = 0x243f6a8885a308d3ull;
        for (size_t k = 0; k < htx.size(); ++k) {
            s = mix64(s + k);
            htx[k] = (unsigned char)s;
            gtx[k] = (unsigned char)(s >> 8);
        }
    }
    ~Link() { free(mb); }
    Link(const Link&) = delete;

    // One call, both sides at once.  cpu_group: the endpoint's group.  lose:
    // 0 none, 1 the GPU's push, 2 the CPU's LL send, 3 the GPU's pull.
    void call(int mode, int cpu_group, long long n, int iters, int check, int nwg, int lose = 0, int lose_at = 2) {
        memset(hrx.data(), 0xEE, hrx.size());
        memset(grx.data(), 0xEE, grx.size());
        const bool unidir = mode == 2;
        Call c;
        c.mb = mb;
        c.tx = htx.data();
        c.rx = hrx.data();
        c.gpu = 3;
        c.mode = mode;
        c.group = cpu_group;
        c.iters = iters;
        c.len = n;
        c.nwg = narrow_nwg(nwg, n);
        c.ll_max = ll_max;
        c.check = check;
        c.expect = checksum(gtx.data(), (size_t)n);
        c.expect_ack = checksum(gtx.data(), 1);
        c.tx_seq0 = c.rx_seq0 = seq;
        if (iters > 0) ++calls;
        c.call = calls;
        c.timeout_s = 5.0;
        c.skip_push = lose == 2 ? lose_at : 0;
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
        g.ll_max = ll_max;
        g.check = check;
        g.expect = checksum(htx.data(), (size_t)n);
        g.expect_ack = checksum(htx.data(), 1);
        g.tx_seq0 = g.rx_seq0 = seq;
        g.call = calls;
        g.lose_push = lose == 1 ? lose_at : 0;
        g.lose_pull = lose == 3 ? lose_at : 0;
        Result r;
        std::thread th(run_gpu, &g);
        const int rc = run(c, &r);
        th.join();
        seq += (uint64_t)iters;
        EXPECT(rc == 0 && !r.timed_out && !g.timed_out);
        // what each side received: B bytes, or the unidir sender's one ack byte
        const long long cpu_recv = (unidir && cpu_group == 1) ? 1 : n;
        const long long gpu_recv = (unidir && cpu_group == 0) ? 1 : n;
        EXPECT(r.recv_done == (uint64_t)iters && g.recv_done == (uint64_t)iters);
        if (iters > 0 && !lose) {
            EXPECT(memcmp(hrx.data(), gtx.data(), (size_t)cpu_recv) == 0);
            EXPECT(memcmp(grx.data(), htx.data(), (size_t)gpu_recv) == 0);
        }
        for (size_t k = (size_t)(iters > 0 ? cpu_recv : 0); k < hrx.size(); ++k)
            if (hrx[k] != 0xEE) { EXPECT(!"a byte past the endpoint's receive changed"); break; }
        for (size_t k = (size_t)(iters > 0 ? gpu_recv : 0); k < grx.size(); ++k)
            if (grx[k] != 0xEE) { EXPECT(!"a byte past the GPU side's receive changed"); break; }
        if (check) {
            const uint64_t cpu_want = (unidir && cpu_group == 1) ? c.expect_ack : c.expect;
            const uint64_t gpu_want = (unidir && cpu_group == 0) ? g.expect_ack : g.expect;
            EXPECT(r.check_iters == (uint64_t)iters);
            // a payload lost on its way to one side fails that side once and the other never
            const bool cpu_loses = lose == 1, gpu_loses = lose == 2 || lose == 3;
            EXPECT(r.check_failures == (cpu_loses ? 1 : 0));
            EXPECT(g.failures == (gpu_loses ? 1 : 0));
            if (!cpu_loses) EXPECT(r.recv_digest == cpu_want * (uint64_t)iters);
            if (!gpu_loses) EXPECT(g.digest == gpu_want * (uint64_t)iters);
        } else {
            EXPECT(r.check_iters == 0 && r.check_failures == 0 && r.recv_digest == 0);
        }
    }
};

int main() {
    // the checksum against its definition, spelled out byte by byte
    for (size_t n : {(size_t)0, (size_t)1, (size_t)7, (size_t)8, (size_t)9, (size_t)17, (size_t)4099}) {
        std::vector<unsigned char> b(n + 3);
        for (size_t k = 0; k < b.size(); ++k) b[k] = (unsigned char)(k * 37 + 11);
        for (size_t off : {(size_t)0, (size_t)3}) {
            uint64_t sum = 0;
            for (size_t k = 0; 8 * k < n; ++k) {
                uint64_t w = 0;
                for (size_t j = 0; j < 8 && 8 * k + j < n; ++j) w |= (uint64_t)b[off + 8 * k + j] << (8 * j);
                sum += mix64(w + (k + 1) * 0x9E3779B97F4A7C15ull);
            }
            EXPECT(checksum(b.data() + off, n) == (sum ^ mix64((uint64_t)n)));
        }
    }
    {   // the poison, form by form: LL every byte the low byte, bulk 16-byte units of the word and a byte tail
        unsigned char b[40];
        const uint64_t w = 0x5a5a5a5a5a5a5a5aull ^ 0x1234ull;
        memset(b, 0, sizeof b);
        poison(b, 37, 0x1234, true);
        for (int k = 0; k < 40; ++k) EXPECT(b[k] == (k < 37 ? (unsigned char)w : 0));
        memset(b, 0, sizeof b);
        poison(b, 37, 0x1234, false);
        for (int k = 0; k < 40; ++k)
            EXPECT(b[k] == (k < 32 ? (unsigned char)(w >> (8 * (k % 8))) : k < 37 ? (unsigned char)w : 0));
    }
    EXPECT(ll_units(0) == 1 && ll_units(1) == 1 && ll_units(8) == 1 && ll_units(9) == 2 && ll_units(8192) == 1024);
    EXPECT(kDefaultLL <= kLLBytes && kDefaultMaxWG <= kWG && narrow_nwg(128, 4161) == 5 && narrow_nwg(7, 1 << 20) == 7 && narrow_nwg(4, 0) == 1);
    EXPECT(ll_tag(1) == 0x80000001u && ll_tag(0x80000000ull) == 0x80000000u);
    EXPECT(ll_tag(0x7fffffffull) == 0xffffffffu && ll_tag(0xffffffffull) == 0xffffffffu);
    EXPECT(ll_tag(1ull << 32) == 0x80000000u && ll_tag((1ull << 32) + 1) == 0x80000001u);

    // both modes, both orientations, sizes on both sides of the threshold, with and without check
    {
        Link l(70016);
        const long long sizes[] = {0, 1, 8, 2045, kDefaultLL, kDefaultLL + 1, 4161, 70001};
        for (int mode : {0, 2})
            for (int cpu_group : {0, 1})
                for (long long n : sizes)
                    for (int check : {0, 1}) l.call(mode, cpu_group, n, check ? 5 : 3, check, n > 60000 ? 7 : 4);
        // a call that moves nothing, then the link goes on
        l.call(0, 1, 4161, 0, 1, 4);
        l.call(0, 0, 8, 1, 1, 4);
        // forced bulk (threshold 0: the ack is pulled and pushed too) and forced LL
        l.ll_max = 0;
        for (int mode : {0, 2})
            for (int cpu_group : {0, 1}) l.call(mode, cpu_group, 777, 4, 1, 3);
        l.ll_max = kLLBytes;
        for (int mode : {0, 2})
            for (int cpu_group : {0, 1}) l.call(mode, cpu_group, 8192, 4, 1, 3);
    }
    // The wrap points.  A link "near P": its next push is number P - 4.  Every
    // case gets a fresh Link (a zeroed mailbox), so no LL message follows a
    // larger one by a multiple of 2^31 pushes (the LL zone's documented alias).
    // The boundary inside one call (9 iterations) and between two (4 + 4: the
    // first call ends on push P - 1); with the call number starting at
    // 2^32 - 2, so the second call of the 4 + 4 form posts 2^32.
    for (uint64_t P : {1ull << 31, 1ull << 32})
        for (int mode : {0, 2})
            for (int cpu_group : {0, 1})
                for (long long n : {8ll, 4161ll})
                    for (uint64_t calls0 : {0ull, (1ull << 32) - 2}) {
                        {
                            Link l(8192);
                            l.seq = P - 5;
                            l.calls = calls0;
                            l.call(mode, cpu_group, n, 9, 1, 4);
                            EXPECT(l.seq == P + 4 && l.calls == calls0 + 1);
                        }
                        {
                            Link l(8192);
                            l.seq = P - 5;
                            l.calls = calls0;
                            l.call(mode, cpu_group, n, 4, 1, 4);
                            EXPECT(l.seq == P - 1);
                            l.call(mode, cpu_group, n, 0, 1, 4);   // (posts nothing, takes no number)
                            l.call(mode, cpu_group, n, 4, 1, 4);
                            l.call(mode, 1 - cpu_group, n, 2, 1, 4);
                            EXPECT(l.seq == P + 5 && l.calls == calls0 + 3);
                        }
                    }
    // a lost payload: the receiver's checksum misses once, the sender's side is clean
    {
        Link l(8192);
        l.call(2, 0, 8, 5, 1, 4, /*lose*/ 1);       // GPU -> CPU, LL
        l.call(2, 0, 4161, 5, 1, 4, 1);             // GPU -> CPU, bulk
        l.call(2, 1, 8, 5, 1, 4, 2);                // CPU -> GPU, LL
        l.call(2, 1, 4161, 5, 1, 4, 3);             // CPU -> GPU, bulk (the pull drops it)
        l.call(0, 1, 4161, 5, 1, 4);                // and the link still works
    }
    // a peer that never comes: every first wait of the endpoint runs into its deadline
    for (int mode : {0, 2})
        for (int group : {0, 1})
            for (long long n : {8ll, 4161ll}) {
                Link l(8192);
                Call c;
                c.mb = l.mb;
                c.tx = l.htx.data();
                c.rx = l.hrx.data();
                c.gpu = 3;
                c.mode = mode;
                c.group = group;
                c.iters = 3;
                c.len = n;
                c.nwg = 4;
                c.call = 1;
                c.timeout_s = 0.02;
                Result r;
                const double t0 = now_s();
                EXPECT(run(c, &r) == 1 && r.timed_out == 1 && r.recv_done == 0);
                EXPECT(now_s() - t0 < 2.0);
            }
    if (g_fail) {
        fprintf(stderr, "hostlink_host_check: %d failures\n", g_fail);
        return 1;
    }
    puts("hostlink_host_check: ok");
    return 0;
}
