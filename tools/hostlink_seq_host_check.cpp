// hostlink_seq_host_check — the CPU endpoint's sequenced loop
// (mpi-perf_amd/csrc/mpx_hostlink.h: run_seq) as a stand-alone program for the
// host sanitizers: tools/asan_hostlink_seq.sh builds it with
// -fsanitize=address,undefined and once more with -fsanitize=thread and runs
// each once.  No GPU, no libmpx: a second CPU thread plays the GPU's side of
// the protocol (what k_hostlink_gen does: generated pushes, polls, pulls and
// credits) on malloc'ed memory.  Covered: both modes, both orientations, sizes
// on both sides of the LL threshold, forced forms, check mode with a checksum
// per payload, what the endpoint's tx holds afterwards, a link across push
// 2^32, the seq_stale knob in both forms, and a GPU side that credits a pull
// (and answers it) BEFORE it loads tx: the ordinary loop cannot show that, the
// sequenced loop shows it as a byte mismatch.
//   With the argument `rate` (an ordinary -O2 build, no sanitizer) it prints
// one JSON line instead: how fast this CPU writes a 4 MiB payload with
// seq::pattern, which is what a sequenced bulk send adds on the endpoint.
#include "mpx_hostlink.h"

#include <stdio.h>
#include <stdlib.h>

#include <thread>
#include <vector>

using namespace mpx::hostlink;
namespace sq = mpx::seq;

static int g_fail = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);      \
            ++g_fail;                                                       \
        }                                                                   \
    } while (0)

static bool same(const unsigned char* a, const unsigned char* b, size_t n) { return n == 0 || memcmp(a, b, n) == 0; }

static const uint64_t kSeed = 0x5EC0DED5EED5EED5ull;
static const int kGpuRank = 3, kHostRank = 20;

// P(seed, s, d, i, n), spelled out byte by byte from the fill's definition
static std::vector<unsigned char> payload(int s, int d, int i, size_t n) {
    const uint64_t key = mpx_pattern_key(kSeed, (unsigned)s, (unsigned)d, (unsigned)i);
    std::vector<unsigned char> b(n);
    for (size_t k = 0; k < n; ++k) b[k] = (unsigned char)(sq::mix64((key ^ (uint64_t)(k / 8)) + sq::kGolden) >> (8 * (k % 8)));
    return b;
}

// ---- the GPU's side, on a CPU thread ----------------------------------------
struct Gpu {
    HostMailbox* mb;
    const unsigned char* host_tx;   // the endpoint's buffers, as the kernel maps them
    unsigned char* host_rx;
    unsigned char* rx;
    int mode, group, iters;
    long long len;
    int nwg, ll_max, check;
    uint64_t tx_seq0, rx_seq0, call;
    bool seq_send = true;      // false: the ordinary kernel's side, sending `plain`
    const unsigned char* plain = nullptr;
    int early = -1;            // the iteration whose pull is credited and answered before tx is loaded
    std::vector<uint64_t> got; // check: the checksum of every received payload
    uint64_t recv_done = 0;
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
    uint64_t txs = g->tx_seq0, rxs = g->rx_seq0;
    st_rel(&in.posted[kGpuRank], g->call);
    if (g->iters > 0 && g->group == 1 && !w.until([&] { return ld_acq(&out.posted[kGpuRank]) >= g->call; })) {
        g->timed_out = 1;
        return;
    }
    auto send = [&](int i) {
        ++txs;
        std::vector<unsigned char> gen;
        const unsigned char* src = g->plain;
        if (g->seq_send) {
            gen = payload(kGpuRank, kHostRank, i, (size_t)send_len);
            src = gen.data();
        }
        if (send_len <= g->ll_max) {
            const uint64_t tag = (uint64_t)ll_tag(txs) << 32;
            for (int k = 0; k < 2 * ll_units(send_len); ++k) {
                uint32_t v = 0;
                const long long off = 4ll * k;
                if (off < send_len) memcpy(&v, src + off, (size_t)(send_len - off < 4 ? send_len - off : 4));
                __atomic_store_n(&in.ll[kGpuRank][k], tag | v, __ATOMIC_RELEASE);
            }
            return;
        }
        for (int k = 0; k < g->nwg; ++k) {
            long long lo, hi;
            chunk_of(send_len, g->nwg, k, &lo, &hi);
            if (lo < hi) memcpy(g->host_rx + lo, src + lo, (size_t)(hi - lo));
            st_rel(&in.flag[kGpuRank][k], txs);
        }
    };
    // the pull of message rxs: every chunk of the endpoint's tx, then its credit
    auto pull = [&]() {
        for (int k = 0; k < g->nwg; ++k) {
            long long lo, hi;
            chunk_of(recv_len, g->nwg, k, &lo, &hi);
            if (lo < hi) memcpy(g->rx + lo, g->host_tx + lo, (size_t)(hi - lo));
        }
    };
    auto credit = [&]() {
        for (int k = 0; k < g->nwg; ++k) st_rel(&in.credit[kGpuRank][k], rxs);
    };
    auto recv = [&](int i) {
        ++rxs;
        if (recv_len <= g->ll_max) {
            const uint32_t tag = ll_tag(rxs);
            for (int k = 0; k < 2 * ll_units(recv_len); ++k) {
                uint64_t v = 0;
                if (!w.until([&] { return (uint32_t)((v = ld_acq(&out.ll[kGpuRank][k])) >> 32) == tag; })) return false;
                const long long off = 4ll * k;
                const uint32_t d = (uint32_t)v;
                if (off < recv_len) memcpy(g->rx + off, &d, (size_t)(recv_len - off < 4 ? recv_len - off : 4));
            }
        } else {
            if (!w.until([&] { return ld_acq(&out.ready[kGpuRank]) >= rxs; })) return false;
            if (i == g->early) {
                // the broken side: the credit first, and (group 0) the answer
                // the endpoint waits for next, so that it goes on to its next
                // send; tx is loaded only once that send is announced
                credit();
                if (g->group == 0) send(i);
                if (!w.until([&] { return ld_acq(&out.ready[kGpuRank]) >= rxs + 1; })) return false;
                pull();
            } else {
                pull();
                credit();
            }
        }
        ++g->recv_done;
        if (g->check) {
            g->got.push_back(checksum(g->rx, (size_t)recv_len));
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
            if (i != g->early) send(i);
        }
    }
}

// ---- one link: an endpoint, a GPU rank, their buffers and counters ------------
struct Link {
    static constexpr size_t kGuard = 64;
    size_t cap;
    HostMailbox* mb;
    std::vector<unsigned char> htx, hrx, gtx, grx, htx0;
    uint64_t seq = 0, calls = 0;
    int ll_max = kDefaultLL;
    explicit Link(size_t cap_) : cap(cap_), htx(cap_ + kGuard), hrx(cap_ + kGuard), gtx(cap_ + kGuard), grx(cap_ + kGuard) {
        mb = static_cast<HostMailbox*>(calloc(1, sizeof(HostMailbox)));
    }
    ~Link() { free(mb); }
    Link(const Link&) = delete;

    // One call, both sides at once.  cpu_group: the endpoint's group.
    // stale: the endpoint's seq_stale knob; early: the GPU side's broken pull;
    // ordinary: the endpoint runs the ordinary loop (its tx is what it sends).
    // Returns the iterations whose payload failed the GPU side's comparison,
    // as a bit mask (check mode).
    uint64_t call(int mode, int cpu_group, long long n, int iters, int check, int nwg, int stale = 0, int early = -1,
                  bool ordinary = false) {
        memset(hrx.data(), 0xEE, hrx.size());
        memset(grx.data(), 0xEE, grx.size());
        uint64_t s = 0x243f6a8885a308d3ull + seq;
        for (size_t k = 0; k < htx.size(); ++k) {   // none of the payloads
            s = mix64(s + k);
            htx[k] = (unsigned char)s;
            gtx[k] = (unsigned char)(s >> 8);
        }
        htx0 = htx;
        const bool unidir = mode == 2;
        const long long cpu_send = (unidir && cpu_group == 0) ? 1 : n, cpu_recv = (unidir && cpu_group == 1) ? 1 : n;
        const long long gpu_recv = cpu_send;
        std::vector<uint64_t> cpu_want, gpu_want;
        for (int i = 0; i < iters; ++i) {
            const std::vector<unsigned char> a = payload(kGpuRank, kHostRank, i, (size_t)cpu_recv);
            const std::vector<unsigned char> b = payload(kHostRank, kGpuRank, i, (size_t)gpu_recv);
            // (the library's own expectation is the same number)
            EXPECT(sq::expect(sq::key_of(sq::key_base(kSeed, kGpuRank, kHostRank), i), a.size()) == checksum(a.data(), a.size()));
            // an ordinary call: each side sends its tx
            cpu_want.push_back(ordinary ? checksum(gtx.data(), (size_t)cpu_recv) : checksum(a.data(), a.size()));
            gpu_want.push_back(ordinary ? checksum(htx0.data(), (size_t)gpu_recv) : checksum(b.data(), b.size()));
        }
        Call c;
        c.mb = mb;
        c.tx = htx.data();
        c.rx = hrx.data();
        c.gpu = kGpuRank;
        c.mode = mode;
        c.group = cpu_group;
        c.iters = iters;
        c.len = n;
        c.nwg = narrow_nwg(nwg, n);
        c.ll_max = ll_max;
        c.check = check;
        c.expect = cpu_want.empty() ? 0 : cpu_want[0];   // (the ordinary loop's one expectation: unused where it matters)
        c.expect_ack = c.expect;
        c.tx_seq0 = c.rx_seq0 = seq;
        if (iters > 0) ++calls;
        c.call = calls;
        c.timeout_s = 5.0;
        c.seq_tx = htx.data();
        c.seq_tx_key = sq::key_base(kSeed, kHostRank, kGpuRank);
        c.expect_each = cpu_want.data();
        c.seq_stale = stale;
        Gpu g{};
        g.mb = mb;
        g.host_tx = htx.data();
        g.host_rx = hrx.data();
        g.rx = grx.data();
        g.mode = mode;
        g.group = 1 - cpu_group;
        g.iters = iters;
        g.len = n;
        g.nwg = c.nwg;
        g.ll_max = ll_max;
        g.check = check;
        g.tx_seq0 = g.rx_seq0 = seq;
        g.call = calls;
        g.early = early;
        g.plain = gtx.data();
        g.seq_send = !ordinary;
        Result r;
        std::thread th(run_gpu, &g);
        const int rc = ordinary ? run(c, &r) : run_seq(c, &r);
        th.join();
        seq += (uint64_t)iters;
        EXPECT(rc == 0 && !r.timed_out && !g.timed_out);
        EXPECT(r.recv_done == (uint64_t)iters && g.recv_done == (uint64_t)iters);
        // the endpoint's rx: the GPU's last payload, then guards
        if (iters > 0) {
            const std::vector<unsigned char> last = payload(kGpuRank, kHostRank, iters - 1, (size_t)cpu_recv);
            EXPECT(same(hrx.data(), ordinary ? gtx.data() : last.data(), (size_t)cpu_recv));
        }
        for (size_t k = (size_t)(iters > 0 ? cpu_recv : 0); k < hrx.size(); ++k)
            if (hrx[k] != 0xEE) { EXPECT(!"a byte past the endpoint's receive changed"); break; }
        for (size_t k = (size_t)(iters > 0 ? gpu_recv : 0); k < grx.size(); ++k)
            if (grx[k] != 0xEE) { EXPECT(!"a byte past the GPU side's receive changed"); break; }
        // the endpoint's tx: the last payload over [0, n) after a bulk send (the
        // one before it where the last send was the stale one), untouched otherwise
        if (!ordinary) {
            std::vector<unsigned char> want_tx = htx0;
            if (cpu_send > ll_max) {
                int last = iters - 1;
                if (stale == iters) --last;
                if (last >= 0) {
                    const std::vector<unsigned char> p = payload(kHostRank, kGpuRank, last, (size_t)cpu_send);
                    if (!p.empty()) memcpy(want_tx.data(), p.data(), p.size());
                }
            }
            EXPECT(want_tx == htx);
        } else {
            EXPECT(htx0 == htx);
        }
        uint64_t bad = 0;
        if (check) {
            EXPECT(r.check_iters == (uint64_t)iters && r.check_failures == 0);   // the GPU's sends are always fresh
            uint64_t dig = 0;
            for (uint64_t x : cpu_want) dig += x;
            EXPECT(r.recv_digest == dig);
            EXPECT(g.got.size() == (size_t)iters);
            for (size_t i = 0; i < g.got.size() && i < 64; ++i)
                if (g.got[i] != gpu_want[i]) bad |= 1ull << i;
        } else {
            EXPECT(r.check_iters == 0 && r.check_failures == 0 && r.recv_digest == 0);
            // unchecked: the GPU side's rx holds what the endpoint sent last
            if (iters > 0 && !ordinary && early < 0) {
                const int last = stale == iters ? iters - 2 : iters - 1;
                const std::vector<unsigned char> p =
                    last >= 0 ? payload(kHostRank, kGpuRank, last, (size_t)gpu_recv)
                              : std::vector<unsigned char>(htx0.begin(), htx0.begin() + (long)gpu_recv);
                EXPECT(same(grx.data(), p.data(), p.size()));
            }
        }
        return bad;
    }
};

static int rate() {
    const size_t n = 4u << 20;
    std::vector<unsigned char> b(n);
    sq::pattern(b.data(), n, 1);   // touch the pages
    double best = 0, sum = 0;
    const int reps = 20;
    for (int k = 0; k < reps; ++k) {
        const double t0 = now_s();
        sq::pattern(b.data(), n, sq::key_of(sq::key_base(kSeed, kHostRank, kGpuRank), k));
        const double gbps = (double)n / (now_s() - t0) / 1e9;
        sum += gbps;
        if (gbps > best) best = gbps;
    }
    printf("{\"item\": \"seq_cpu_generation\", \"what\": \"seq::pattern into ordinary memory, one thread\", \"bytes\": %zu, "
           "\"reps\": %d, \"GBps_best\": %.2f, \"GBps_mean\": %.2f, \"last_byte\": %d}\n",
           n, reps, best, sum / reps, (int)b[n - 1]);
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "rate")) return rate();
    // the pattern and its checksum against the fill's definition
    for (size_t n : {(size_t)0, (size_t)1, (size_t)7, (size_t)8, (size_t)9, (size_t)17, (size_t)4099}) {
        const std::vector<unsigned char> want = payload(9, 63, 5, n);
        std::vector<unsigned char> got(n + 8, 0xEE);
        const uint64_t key = sq::key_of(sq::key_base(kSeed, 9, 63), 5);
        EXPECT(key == mpx_pattern_key(kSeed, 9, 63, 5));
        sq::pattern(got.data() + 3, n, key);
        EXPECT(same(got.data() + 3, want.data(), n) && got[n + 3] == 0xEE && got[2] == 0xEE);
        EXPECT(sq::expect(key, n) == checksum(want.data(), n));
    }
    // both modes, both orientations, sizes on both sides of the threshold, with and without check
    {
        Link l(70016);
        const long long sizes[] = {0, 1, 8, 255, kDefaultLL, kDefaultLL + 1, 2045, 4161, 70001};
        for (int mode : {0, 2})
            for (int cpu_group : {0, 1})
                for (long long n : sizes)
                    for (int check : {0, 1})
                        EXPECT(l.call(mode, cpu_group, n, check ? 5 : 3, check, n > 60000 ? 7 : 4) == 0);
        // a call that moves nothing, a single iteration, then the link goes on
        EXPECT(l.call(0, 1, 4161, 0, 1, 4) == 0);
        EXPECT(l.call(0, 0, 8, 1, 1, 4) == 0);
        // sequenced and ordinary calls alternate on one link
        EXPECT(l.call(0, 1, 4161, 3, 1, 4, 0, -1, true) == 0);
        EXPECT(l.call(2, 1, 4161, 3, 1, 4) == 0);
        // forced bulk (threshold 0: the ack and the 0-byte payload are pulled too) and forced LL
        l.ll_max = 0;
        for (int mode : {0, 2})
            for (int cpu_group : {0, 1})
                for (long long n : {0ll, 8ll, 777ll}) EXPECT(l.call(mode, cpu_group, n, 4, 1, 3) == 0);
        l.ll_max = kLLBytes;
        for (int mode : {0, 2})
            for (int cpu_group : {0, 1})
                for (long long n : {8185ll, 8192ll}) EXPECT(l.call(mode, cpu_group, n, 4, 1, 3) == 0);
    }
    // a link whose pushes cross 2^31 and 2^32 inside a 9-iteration call
    for (uint64_t P : {1ull << 31, 1ull << 32})
        for (int mode : {0, 2})
            for (int cpu_group : {0, 1})
                for (long long n : {8ll, 4161ll}) {
                    Link l(8192);
                    l.seq = P - 5;
                    EXPECT(l.call(mode, cpu_group, n, 9, 1, 4) == 0);
                    EXPECT(l.seq == P + 4);
                }
    // seq_stale = k: the GPU side's comparison misses exactly payload k - 1, in both forms,
    // and the call completes; for k = iters the unchecked rx holds payload iters - 2
    {
        Link l(8192);
        for (int mode : {0, 2})
            for (long long n : {8ll, 4161ll})
                for (int k : {1, 2, 5, 9}) {
                    EXPECT(l.call(mode, 1, n, 9, 1, 4, k) == 1ull << (k - 1));
                    EXPECT(l.call(mode, 1, n, 9, 0, 4, k) == 0);
                }
        EXPECT(l.call(0, 0, 4161, 9, 1, 4, 3) == 1ull << 2);   // the endpoint receives first
        EXPECT(l.call(0, 1, 4161, 5, 1, 4) == 0);              // and the link still works
    }
    // A GPU side that credits pull k (and, where the endpoint waits for it,
    // answers it) before it loads tx, and loads once the endpoint has announced
    // message k + 1.  Under the ordinary loop tx never changes, so nothing
    // differs; under the sequenced loop the endpoint has by then written
    // payload k + 1 into tx, and the comparison of iteration k fails.
    {
        Link l(8192);
        for (int mode : {0, 2}) {
            EXPECT(l.call(mode, 1, 4161, 6, 1, 4, 0, /*early*/ 2, /*ordinary*/ true) == 0);
            EXPECT(l.call(mode, 1, 4161, 6, 1, 4, 0, /*early*/ 2) == 1ull << 2);
        }
        EXPECT(l.call(0, 1, 4161, 5, 1, 4) == 0);
    }
    if (g_fail) {
        fprintf(stderr, "hostlink_seq_host_check: %d failures\n", g_fail);
        return 1;
    }
    puts("hostlink_seq_host_check: ok");
    return 0;
}
