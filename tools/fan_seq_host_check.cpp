// fan_seq_host_check — the arithmetic of the sequenced fan payloads
// (mpx_xfer_fan_seq) as a stand-alone program for the host sanitizers
// (tests/test_fan_seq_abi.py builds it with -fsanitize=address,undefined and
// runs it once; no GPU, no libmpx, nothing loaded into python).  It includes
// the host side of the pattern (mpi-perf_amd/csrc/mpx_seq.h) only and restates
// the kernels' side here:
//   * k_xfer_fan's GEN branch: workgroup w of a link nwg wide owns chunk
//     [lo, hi) of the block, generates nv 16-B units from word k0 = lo / 8 on,
//     lane t taking units t, t + 256, ..., and lanes t < tail one tail byte
//     each; for widths 1 - 256 and the block sizes of the tests the units and
//     tail bytes of all workgroups and lanes reassemble to pattern(key, n),
//     every byte written exactly once;
//   * k_xfer_fan_ll's GEN branch: an LL fan message fills half a row (4096 B
//     = 512 8-B units, kUnits = 2 per lane), lane t owning units t and t + 256,
//     the unit that n ends in masked; what push_ll then sends is pattern(key,
//     n) and zero up to the unit's end;
//   * the key both kernels derive, seed ^ me << 56 ^ peer << 48 ^ i << 24, is
//     key_of(key_base(seed, me, peer), i), and all of a rank's links and
//     iterations have keys of their own;
//   * an npeers x iters expectation array is laid out k * iters + i.
// The first mismatch prints and exits 1; otherwise one "ok" line.
#include "mpx_seq.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

using namespace mpx;

#define REQUIRE(cond)                                                        \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: %s is false\n", __FILE__, __LINE__, #cond); \
            return 1;                                                        \
        }                                                                    \
    } while (0)

static const int kBlock = 256;            // lanes of a workgroup
static const int kFanLLUnits = 2;         // Loop<., ANYWG = true>::kUnits: half a row's units per lane
static const size_t kFanLLMax = 4096;     // MPX_FAN_LL_MAX

static const size_t kBulkSizes[] = {0, 1, 15, 16, 17, 2045, 4161, 65555, 71681, 262165};
static const size_t kLLSizes[] = {0, 1, 7, 8, 9, 2045, 4095, 4096};

// a bulk push of one link's block at width nwg, workgroup by workgroup and lane by lane
static int check_bulk(size_t n, int nwg, uint64_t key, const unsigned char* want) {
    std::vector<unsigned char> rx(n, 0xEE);
    std::vector<unsigned char> hits(n, 0);
    const long long N = (long long)n;
    const long long chunk = (((N + nwg - 1) / nwg) + 15) & ~15ll;
    for (int w = 0; w < nwg; ++w) {
        const long long lo = (long long)w * chunk;
        const long long hi = lo + chunk < N ? lo + chunk : N;
        const unsigned bytes = lo < hi ? (unsigned)(hi - lo) : 0u;
        if (!bytes) continue;                     // an empty chunk generates nothing
        const int nv = (int)(bytes >> 4);
        const unsigned tail = bytes & 15;
        const uint64_t k0 = (uint64_t)lo >> 3;
        REQUIRE(lo % 16 == 0);
        REQUIRE(tail == 0 || hi == N);            // only the block's last chunk has a tail
        for (int t = 0; t < kBlock; ++t) {
            for (int v = t; v < nv; v += kBlock) {             // gen_units: the 4-deep batches visit these units
                const uint64_t w0 = seq::fill_word(key, k0 + 2 * (uint64_t)v);
                const uint64_t w1 = seq::fill_word(key, k0 + 2 * (uint64_t)v + 1);
                const size_t at = (size_t)lo + 16 * (size_t)v;
                REQUIRE(at + 16 <= n);
                memcpy(&rx[at], &w0, 8);
                memcpy(&rx[at + 8], &w1, 8);
                for (int b = 0; b < 16; ++b) ++hits[at + b];
            }
            if ((unsigned)t < tail) {                          // the one or two words the tail bytes fall in
                const unsigned o = (unsigned)nv * 16 + (unsigned)t;
                const uint64_t wd = seq::fill_word(key, k0 + (o >> 3));
                REQUIRE((size_t)lo + o < n);
                rx[(size_t)lo + o] = (unsigned char)(wd >> (8 * (o & 7)));
                ++hits[(size_t)lo + o];
            }
        }
    }
    REQUIRE(n == 0 || memcmp(rx.data(), want, n) == 0);
    for (size_t b = 0; b < n; ++b) REQUIRE(hits[b] == 1);
    return 0;
}

// an LL fan push of n bytes: gen_ll's registers, then the units push_ll sends
static int check_ll(size_t n, uint64_t key, const unsigned char* want) {
    REQUIRE(n <= kFanLLMax);
    const int ng = n > 0 ? (int)((n + 3) >> 2) : 1, nu = (ng + 1) >> 1;
    REQUIRE(nu <= kBlock * kFanLLUnits);          // half a row holds the message
    std::vector<unsigned char> rx(8 * (size_t)nu, 0xEE);
    std::vector<unsigned char> sent(nu, 0);
    for (int t = 0; t < kBlock; ++t) {
        uint64_t pre[kFanLLUnits];
        for (int j = 0; j < kFanLLUnits; ++j) {   // gen_ll
            const int u = t + j * kBlock;
            const long long off = 8ll * u;
            uint64_t w = 0;
            if (off < (long long)n) {
                w = seq::fill_word(key, (uint64_t)u);
                if (off + 8 > (long long)n) w &= (1ull << (8 * (int)((long long)n - off))) - 1;
            }
            pre[j] = w;
        }
        for (int j = 0; j < kFanLLUnits; ++j) {   // push_ll
            const int u = t + j * kBlock;
            if (u < nu) {
                memcpy(&rx[8 * (size_t)u], &pre[j], 8);
                ++sent[u];
            }
        }
    }
    for (int u = 0; u < nu; ++u) REQUIRE(sent[u] == 1);
    REQUIRE(n == 0 || memcmp(rx.data(), want, n) == 0);
    for (size_t b = n; b < 8 * (size_t)nu; ++b) REQUIRE(rx[b] == 0);
    return 0;
}

static int check_kernel_views() {
    const uint64_t key = seq::key_of(seq::key_base(MPX_PATTERN_SEED, 9, 63), 32);
    for (size_t n : kBulkSizes) {
        std::vector<unsigned char> want(n);
        seq::pattern(want.data(), n, key);
        for (int nwg = 1; nwg <= 256; ++nwg)
            if (check_bulk(n, nwg, key, want.data())) return 1;
    }
    for (size_t n : kLLSizes) {
        std::vector<unsigned char> want(n);
        seq::pattern(want.data(), n, key);
        if (check_ll(n, key, want.data())) return 1;
    }
    return 0;
}

// the key the kernels derive from FanArgs.seq_seed, my_slot and the link's peer
static uint64_t kernel_key(uint64_t seed, int me, int peer, int i) {
    return seed ^ ((uint64_t)(unsigned)me << 56) ^ ((uint64_t)(unsigned)peer << 48) ^ ((uint64_t)(unsigned)i << 24);
}

static int check_keys_and_layout() {
    const uint64_t seed = 0x0123456789abcdefull;
    std::set<uint64_t> keys;
    const int ranks[] = {0, 1, 9, 40, 63};
    const int iters[] = {0, 1, 2, 32, 255, 1 << 20};
    size_t count = 0;
    for (int me : ranks)
        for (int peer : ranks)
            for (int i : iters) {
                if (me == peer) continue;
                const uint64_t k = kernel_key(seed, me, peer, i);
                REQUIRE(k == seq::key_of(seq::key_base(seed, me, peer), i));
                REQUIRE(k == mpx_pattern_key(seed, (unsigned)me, (unsigned)peer, (unsigned)i));
                keys.insert(k);
                ++count;
            }
    REQUIRE(keys.size() == count);
    // expect[k * iters + i] = checksum of P(seed, peers[k], me, i, n), in the caller's order of peers
    const int me = 2, peers[] = {5, 0, 63}, npeers = 3, its = 7;
    const size_t n = 2045;
    std::vector<uint64_t> expect((size_t)npeers * its);   // exact size: an index past it is the sanitizer's
    for (int k = 0; k < npeers; ++k) {
        const uint64_t base = seq::key_base(seed, peers[k], me);
        for (int i = 0; i < its; ++i) expect[(size_t)k * its + i] = seq::expect(seq::key_of(base, i), n);
    }
    std::set<uint64_t> distinct(expect.begin(), expect.end());
    REQUIRE(distinct.size() == expect.size());
    for (size_t j = 0; j < expect.size(); ++j) {
        const int k = (int)(j / its), i = (int)(j % its);
        REQUIRE(expect[j] == seq::expect(mpx_pattern_key(seed, (unsigned)peers[k], (unsigned)me, (unsigned)i), n));
    }
    return 0;
}

int main() {
    if (check_kernel_views() || check_keys_and_layout()) return 1;
    printf("fan_seq_host_check: ok\n");
    return 0;
}
