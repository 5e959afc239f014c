// seq_host_check — the host side of the sequenced payloads
// (mpi-perf_amd/csrc/mpx_seq.h) as a stand-alone program for the host
// sanitizers (tests/test_seq_abi.py builds it with -fsanitize=address,undefined
// and runs it once; no GPU, no libmpx, nothing loaded into python):
//   * seq::pattern writes exactly n bytes, at any alignment, and they are the
//     words of a restatement of MPX_FILL_SPLITMIX written here;
//   * seq::expect, which never materialises the bytes, is the checksum of those
//     bytes as the endpoint's checksum (mpx_hostlink.h) computes it;
//   * the kernels' view of the same pattern: a bulk chunk's 16-B units and tail
//     bytes (Loop::gen_units, push_bulk) and an LL message's masked 8-B units
//     (Loop::gen_ll), restated here word for word, rebuild the same bytes for
//     every width;
//   * key_of(key_base(...), i) is mpx_pattern_key(..., i).
// The first mismatch prints and exits 1; otherwise one "ok" line.
#include "mpx_seq.h"
#include "mpx_hostlink.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace mpx;

#define REQUIRE(cond)                                                        \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: %s is false\n", __FILE__, __LINE__, #cond); \
            return 1;                                                        \
        }                                                                    \
    } while (0)

static uint64_t splitmix(uint64_t key, uint64_t k) {
    uint64_t z = (key ^ k) + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

static const size_t kSizes[] = {0, 1, 7, 8, 9, 13, 15, 16, 17, 2045, 2048, 2049, 4097, 4161, 65537, 71681, 262165};
static const int kIters[] = {0, 1, 2, 255, 256, 1 << 24, 0x7fffffff};

static int check_pattern_and_expect() {
    for (size_t n : kSizes)
        for (int it : kIters)
            for (size_t off : {(size_t)0, (size_t)1, (size_t)3, (size_t)8}) {
                const uint64_t key = seq::key_of(seq::key_base(0x1234567890abcdefull, 9, 63), it);
                REQUIRE(key == mpx_pattern_key(0x1234567890abcdefull, 9, 63, (unsigned)it));
                // an exact-size heap block: a byte written past n, or before off, is the sanitizer's
                std::vector<unsigned char> buf(off + n);
                seq::pattern(buf.data() + off, n, key);
                for (size_t b = 0; b < n; ++b)
                    REQUIRE(buf[off + b] == (unsigned char)(splitmix(key, b / 8) >> (8 * (b % 8))));
                REQUIRE(seq::expect(key, n) == hostlink::checksum(buf.data() + off, n));
            }
    return 0;
}

// a bulk push of n bytes at width nwg, as the kernels cut and generate it
static int check_bulk(size_t n, int nwg, uint64_t key, const unsigned char* want) {
    std::vector<unsigned char> rx(n, 0xEE);
    const size_t chunk = (((n + (size_t)nwg - 1) / (size_t)nwg) + 15) & ~(size_t)15;   // Loop::chunk_of
    for (int w = 0; w < nwg; ++w) {
        const size_t lo = (size_t)w * chunk, hi = lo + chunk < n ? lo + chunk : n;
        if (lo >= hi) continue;
        const size_t bytes = hi - lo, nv = bytes >> 4, k0 = lo >> 3;
        for (size_t v = 0; v < nv; ++v) {           // gen16: words k0 + 2v and k0 + 2v + 1
            const uint64_t w0 = seq::fill_word(key, k0 + 2 * v), w1 = seq::fill_word(key, k0 + 2 * v + 1);
            memcpy(&rx[lo + 16 * v], &w0, 8);
            memcpy(&rx[lo + 16 * v + 8], &w1, 8);
        }
        for (size_t t = 0; t < (bytes & 15); ++t) { // the tail: the one or two words its bytes fall in
            const size_t o = nv * 16 + t;
            rx[lo + o] = (unsigned char)(seq::fill_word(key, k0 + (o >> 3)) >> (8 * (o & 7)));
        }
    }
    REQUIRE(n == 0 || memcmp(rx.data(), want, n) == 0);
    return 0;
}

// an LL message of n bytes: unit u carries bytes [8u, 8u + 8), zero past n
static int check_ll(size_t n, uint64_t key, const unsigned char* want) {
    const size_t ng = n > 0 ? (n + 3) >> 2 : 1, nu = (ng + 1) >> 1;
    std::vector<unsigned char> rx(8 * nu, 0xEE);
    for (size_t u = 0; u < nu; ++u) {
        const size_t off = 8 * u;
        uint64_t w = 0;
        if (off < n) {
            w = seq::fill_word(key, u);
            if (off + 8 > n) w &= (1ull << (8 * (int)(n - off))) - 1;
        }
        memcpy(&rx[off], &w, 8);
    }
    REQUIRE(n == 0 || memcmp(rx.data(), want, n) == 0);
    for (size_t b = n; b < 8 * nu; ++b) REQUIRE(rx[b] == 0);
    return 0;
}

static int check_kernel_views() {
    for (size_t n : kSizes) {
        const uint64_t key = seq::key_of(seq::key_base(MPX_PATTERN_SEED, 1, 0), 33);
        std::vector<unsigned char> want(n);
        seq::pattern(want.data(), n, key);
        for (int nwg : {1, 2, 5, 7, 17, 70, 128, 256})
            if (check_bulk(n, nwg, key, want.data())) return 1;
        if (n <= 8192 && check_ll(n, key, want.data())) return 1;
    }
    return 0;
}

int main() {
    if (check_pattern_and_expect() || check_kernel_views()) return 1;
    printf("seq_host_check: ok\n");
    return 0;
}
