// hostlink_duplex_host_check — the CPU endpoint's side of the host link's
// full-duplex loop (mpi-perf_amd/csrc/mpx_hostlink.h: run_duplex) as a
// stand-alone program for the host sanitizers: tools/asan_hostlink_duplex.sh
// builds it with -fsanitize=address,undefined and once more with
// -fsanitize=thread and runs each once.  No GPU, no libmpx: a second CPU
// thread plays the kernel's side of the same protocol (what k_hostlink_duplex
// does with its two halves: posted, pushes and flags on the publish schedule,
// the ready word, pulls and credits, the window flush, check mode's one-slot
// ring) on malloc'ed memory.  Covered: iterations 0, 1, 255, 256, 257 and
// 512; sizes 0, 8 and 4161 at widths 1 and 3; check mode on and off; the
// publish schedules 1, 16 and 256; a lost payload in each direction; links
// that start 4 short of push 2^32 and of call 2^32; a peer that never comes.
//   With arguments it prints "<iters> <recv_done>" of an unchecked 8-byte
// call for each iteration count given (tests/test_hostlink_duplex_abi.py
// holds the window arithmetic to iters - iters / 256 with it).
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

// ---- the kernel's side, on a CPU thread ---------------------------------------
struct Gpu {
    HostMailbox* mb;
    const unsigned char* host_tx;   // the endpoint's buffers, as the kernel maps them
    unsigned char* host_rx;
    const unsigned char* tx;        // the GPU rank's own
    unsigned char* rx;
    int gpu, iters;
    long long len;
    int nwg, check, nb_publish;
    uint64_t expect, tx_seq0, rx_seq0, call;
    int lose = 0;                   // 1 + the iteration whose payload is lost, in each direction
    uint64_t recv_done = 0, digest = 0, check_iters = 0;
    int failures = 0, timed_out = 0;
};

static void chunk_of(long long n, int nwg, int w, long long* lo, long long* hi) {
    const long long chunk = (((n + nwg - 1) / nwg) + 15) & ~15ll;
    *lo = (long long)w * chunk;
    *hi = *lo + chunk < n ? *lo + chunk : n;
}

// Both halves of the kernel's grid as one cooperative loop: the pushing half
// has done p iterations, the pulling half q; each advances when its own wait
// would end.  Neither starts the first iteration of a window before both have
// finished slots 0..254 of the one before (the flush).
static void run_gpu(Gpu* g) {
    HostBox& in = g->mb->in;
    HostBox& out = g->mb->out;
    st_rel(&in.posted[g->gpu], g->call);
    int p = 0, q = 0;
    bool posted = false;
    double t0 = now_s();
    auto publishes = [&](int i) {
        return (i + 1) % g->nb_publish == 0 || i % 256 == 254 || i + 1 == g->iters;
    };
    auto gate = [&](int i) { return i % 256 != 0 || i == 0 || (p >= i - 1 && q >= i - 1); };
    while (p < g->iters || q < g->iters) {
        bool moved = false;
        if (p < g->iters && gate(p)) {                  // the pushing half
            if (!posted) posted = ld_acq(&out.posted[g->gpu]) >= g->call;
            const bool credited = !g->check || p == 0 || ld_acq(&out.credit[g->gpu][0]) >= g->tx_seq0 + (uint64_t)p;
            if (posted && credited) {
                const uint64_t seq = g->tx_seq0 + (uint64_t)p + 1;
                for (int k = 0; k < g->nwg; ++k) {
                    long long lo, hi;
                    chunk_of(g->len, g->nwg, k, &lo, &hi);
                    if (lo < hi && g->lose != p + 1) memcpy(g->host_rx + lo, g->tx + lo, (size_t)(hi - lo));
                }
                if (g->check || publishes(p))
                    for (int k = 0; k < g->nwg; ++k) st_rel(&in.flag[g->gpu][k], seq);
                ++p;
                moved = true;
            }
        }
        if (q < g->iters && gate(q)) {                  // the pulling half
            const uint64_t seq = g->rx_seq0 + (uint64_t)q + 1;
            if (ld_acq(&out.ready[g->gpu]) >= seq) {
                for (int k = 0; k < g->nwg; ++k) {
                    long long lo, hi;
                    chunk_of(g->len, g->nwg, k, &lo, &hi);
                    if (lo < hi && g->lose != q + 1) memcpy(g->rx + lo, g->host_tx + lo, (size_t)(hi - lo));
                }
                if (g->check) {
                    const uint64_t got = checksum(g->rx, (size_t)g->len);
                    if (q % 256 != 255) g->digest += got;
                    ++g->check_iters;
                    if (got != g->expect) ++g->failures;
                    if (q + 1 != g->iters) poison(g->rx, (size_t)g->len, q, false);
                }
                if (publishes(q))
                    for (int k = 0; k < g->nwg; ++k) st_rel(&in.credit[g->gpu][k], seq);
                ++q;
                moved = true;
            }
        }
        if (moved) {
            t0 = now_s();
        } else {
            if (now_s() - t0 > 5.0) {
                g->timed_out = 1;
                return;
            }
            cpu_pause();
        }
    }
    g->recv_done = (uint64_t)(g->iters - g->iters / 256);
}

// ---- one link: an endpoint, a GPU rank, their buffers and counters ------------
struct Link {
    static constexpr size_t kGuard = 64;
    size_t cap;
    HostMailbox* mb;
    std::vector<unsigned char> htx, hrx, gtx, grx;
    uint64_t seq = 0, calls = 0;
    int nb_publish = 16;
    uint64_t last_recv_done = 0;
    explicit Link(size_t cap_) : cap(cap_), htx(cap_ + kGuard), hrx(cap_ + kGuard), gtx(cap_ + kGuard), grx(cap_ + kGuard) {
        mb = static_cast<HostMailbox*>(calloc(1, sizeof(HostMailbox)));
        uint64_t s = 0x13198a2e03707344ull;
        for (size_t k = 0; k < htx.size(); ++k) {
            s = mix64(s + k);
            htx[k] = (unsigned char)s;
            gtx[k] = (unsigned char)(s >> 8);
        }
    }
    ~Link() { free(mb); }
    Link(const Link&) = delete;

    // one call, both sides at once; lose: 1 + the iteration whose payload the kernel's side loses, each way
    void call(long long n, int iters, int check, int nwg, int lose = 0) {
        memset(hrx.data(), 0xEE, hrx.size());
        memset(grx.data(), 0xEE, grx.size());
        Call c;
        c.mb = mb;
        c.tx = htx.data();
        c.rx = hrx.data();
        c.gpu = 3;
        c.iters = iters;
        c.len = n;
        c.nwg = narrow_nwg(nwg, n);
        c.check = check;
        c.expect = checksum(gtx.data(), (size_t)n);
        c.tx_seq0 = c.rx_seq0 = seq;
        if (iters > 0) ++calls;
        c.call = calls;
        c.timeout_s = 5.0;
        Gpu g{};
        g.mb = mb;
        g.host_tx = htx.data();
        g.host_rx = hrx.data();
        g.tx = gtx.data();
        g.rx = grx.data();
        g.gpu = 3;
        g.iters = iters;
        g.len = n;
        g.nwg = c.nwg;
        g.check = check;
        g.nb_publish = nb_publish;
        g.expect = checksum(htx.data(), (size_t)n);
        g.tx_seq0 = g.rx_seq0 = seq;
        g.call = calls;
        g.lose = lose;
        Result r;
        std::thread th(run_gpu, &g);
        const int rc = run_duplex(c, &r);
        th.join();
        seq += (uint64_t)iters;
        last_recv_done = r.recv_done;
        EXPECT(rc == 0 && !r.timed_out && !g.timed_out);
        const uint64_t counted = (uint64_t)(iters - iters / 256);
        EXPECT(r.recv_done == counted && g.recv_done == counted);
        if (iters > 0 && !(lose == iters)) {   // (the last payload lost: rx holds the poison, or the guard)
            EXPECT(memcmp(hrx.data(), gtx.data(), (size_t)n) == 0);
            EXPECT(memcmp(grx.data(), htx.data(), (size_t)n) == 0);
        }
        for (size_t k = (size_t)(iters > 0 ? n : 0); k < hrx.size(); ++k)
            if (hrx[k] != 0xEE) { EXPECT(!"a byte past the endpoint's receive changed"); break; }
        for (size_t k = (size_t)(iters > 0 ? n : 0); k < grx.size(); ++k)
            if (grx[k] != 0xEE) { EXPECT(!"a byte past the GPU side's receive changed"); break; }
        // the link's words as a call leaves them: every send pulled, every payload flagged
        for (int k = 0; k < c.nwg && iters > 0; ++k) {
            EXPECT(ld_acq(&mb->in.flag[3][k]) == seq);
            EXPECT(ld_acq(&mb->in.credit[3][k]) == seq);
        }
        if (iters > 0) EXPECT(ld_acq(&mb->out.ready[3]) == seq && ld_acq(&mb->out.posted[3]) == calls);
        if (check) {
            EXPECT(r.check_iters == (uint64_t)iters && g.check_iters == (uint64_t)iters);
            const int lost = (lose >= 1 && lose <= iters) ? 1 : 0;
            EXPECT(r.check_failures == lost && g.failures == lost);
            if (!lost) {
                EXPECT(r.recv_digest == c.expect * counted);
                EXPECT(g.digest == g.expect * counted);
            }
            if (iters > 0) EXPECT(ld_acq(&mb->out.credit[3][0]) == seq);
        } else {
            EXPECT(r.check_iters == 0 && r.check_failures == 0 && r.recv_digest == 0);
        }
    }
};

int main(int argc, char** argv) {
    if (argc > 1) {   // the window arithmetic, for the caller to judge
        for (int k = 1; k < argc; ++k) {
            Link l(64);
            const int iters = atoi(argv[k]);
            l.call(8, iters, 0, 1);
            printf("%d %llu\n", iters, (unsigned long long)l.last_recv_done);
        }
        return g_fail ? 1 : 0;
    }
    const int iterations[] = {0, 1, 255, 256, 257, 512};
    {   // every iteration count, size and width, unchecked and checked, on ONE link
        Link l(8192);
        for (int iters : iterations)
            for (long long n : {0ll, 8ll, 4161ll})
                for (int nwg : {1, 3})
                    for (int check : {0, 1}) l.call(n, iters, check, nwg);
    }
    // the publish schedule's ends: every push and receive published, and none but slot 254 and the last
    for (int every : {1, 256}) {
        Link l(8192);
        l.nb_publish = every;
        for (int iters : {1, 255, 256, 257, 512})
            for (int check : {0, 1}) l.call(4161, iters, check, 3);
    }
    // a lost payload in each direction (the kernel's side loses both): one failure on either end
    {
        Link l(8192);
        l.call(4161, 5, 1, 3, /*lose*/ 2);
        l.call(8, 5, 1, 1, 2);
        l.call(4161, 257, 1, 3, 256);     // an uncounted receive (slot 255) is checked too
        l.call(4161, 5, 0, 3, 2);         // unchecked: unseen
        l.call(4161, 5, 1, 3);            // and the link still works
    }
    // The wrap points: a link whose next push is number 2^32 - 4, the boundary
    // inside one call and between two; and a link 2 calls short of call 2^32.
    for (int check : {0, 1})
        for (long long n : {8ll, 4161ll}) {
            {
                Link l(8192);
                l.seq = (1ull << 32) - 5;
                l.call(n, 33, check, 3);
                EXPECT(l.seq == (1ull << 32) + 28);
                l.call(n, 257, check, 3);
            }
            {
                Link l(8192);
                l.seq = (1ull << 32) - 5;
                l.calls = (1ull << 32) - 2;
                l.call(n, 4, check, 3);
                EXPECT(l.seq == (1ull << 32) - 1 && l.calls == (1ull << 32) - 1);
                l.call(n, 0, check, 3);   // (posts nothing, takes no number)
                l.call(n, 4, check, 3);
                l.call(n, 2, check, 3);
                EXPECT(l.seq == (1ull << 32) + 5 && l.calls == (1ull << 32) + 1);
            }
        }
    // a peer that never comes: the endpoint's flush or final wait runs into its deadline
    for (int iters : {3, 300})
        for (int check : {0, 1}) {
            Link l(8192);
            Call c;
            c.mb = l.mb;
            c.tx = l.htx.data();
            c.rx = l.hrx.data();
            c.gpu = 3;
            c.iters = iters;
            c.len = 4161;
            c.nwg = 3;
            c.check = check;
            c.call = 1;
            c.timeout_s = 0.02;
            Result r;
            const double t0 = now_s();
            EXPECT(run_duplex(c, &r) == 1 && r.timed_out == 1 && r.recv_done == 0);
            EXPECT(r.where == (iters > 255 ? 255 : iters - 1));
            EXPECT(now_s() - t0 < 2.0);
        }
    if (g_fail) {
        fprintf(stderr, "hostlink_duplex_host_check: %d failures\n", g_fail);
        return 1;
    }
    puts("hostlink_duplex_host_check: ok");
    return 0;
}
