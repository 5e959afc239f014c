// copy_window_host_check — k_copy's resident-window rule and its knob
// (copy_window_rule, copy_window_parse: mpx_internal.h) as a stand-alone
// program for the host sanitizers; no GPU, no libmpx:
//   g++ -std=c++17 -fsanitize=address,undefined -D__HIP_PLATFORM_AMD__ \
//       -I$ROCM/include -Impi-perf_amd/csrc tools/copy_window_host_check.cpp
// The first property that does not hold prints and exits 1.
#include "mpx_internal.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace mpx;

#define REQUIRE(cond)                                                        \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: %s is false (n = %zu)\n", __FILE__, __LINE__, #cond, n); \
            return 1;                                                        \
        }                                                                    \
    } while (0)

static bool pow2(unsigned x) { return x && !(x & (x - 1)); }

// bytes of [0, n) the window keeps, restated block by block over one period
static size_t resident_bytes(const CopyWindow& w, size_t n) {
    if (!w.on) return 0;
    const size_t unit_bytes = (size_t)w.unit * kCopyBlockBytes, period_bytes = unit_bytes * w.period;
    const size_t kept_bytes = unit_bytes * w.window;
    const size_t whole = n / period_bytes, rest = n % period_bytes;
    return whole * kept_bytes + (rest < kept_bytes ? rest : kept_bytes);
}

static int check_rule() {
    const size_t MiB = (size_t)1 << 20;
    const size_t period_bytes = (size_t)kCopyWindowUnit * kCopyWindowPeriod * kCopyBlockBytes;
    std::vector<size_t> sizes = {0, 1, 15, 16, 4095, 4096, 4097, MiB, 16 * MiB, 256 * MiB};
    // around the threshold, around every count of periods at which the window
    // changes, and around the size at which one unit per period passes the cap
    const size_t marks[] = {kCopyWindowMin, kCopyWindowCap, 768 * MiB, 1024 * MiB, 1536 * MiB, 2048 * MiB, 3072 * MiB,
                            4096 * MiB, kCopyWindowCap * kCopyWindowPeriod, kCopyWindowCap * kCopyWindowPeriod * 2,
                            (size_t)1 << 40};
    for (size_t m : marks)
        for (long long d : {-(long long)period_bytes, -4097ll, -4096ll, -1ll, 0ll, 1ll, 13ll, 4096ll, 4097ll, (long long)period_bytes})
            if ((long long)m + d >= 0) sizes.push_back((size_t)((long long)m + d));
    for (size_t k = 1; k <= 200; ++k) {
        sizes.push_back(k * period_bytes);
        sizes.push_back(k * period_bytes + 1);
    }
    std::sort(sizes.begin(), sizes.end());
    bool seen_on = false, seen_off_after_on = false;
    unsigned last_window = ~0u;
    for (size_t n : sizes) {
        const CopyWindow w = copy_window_rule(n);
        if (n < kCopyWindowMin) REQUIRE(!w.on);
        if (!w.on) {
            REQUIRE(w.window == 0);
            if (seen_on) seen_off_after_on = true;
            continue;
        }
        REQUIRE(!seen_off_after_on);                       // one range of sizes has the window on
        seen_on = true;
        REQUIRE(pow2(w.unit) && pow2(w.period));
        REQUIRE(w.window >= 1 && w.window <= w.period);
        REQUIRE(resident_bytes(w, n) <= kCopyWindowCap);
        REQUIRE(w.window <= last_window);                  // a larger copy never keeps a larger share
        last_window = w.window;
    }
    size_t n = (size_t)1 << 30;                            // the headline's size: the lab's form win_PL_W192_u1M
    const CopyWindow h = copy_window_rule(n);
    REQUIRE(h.on && h.unit == 256 && h.period == 32 && h.window == 6 && resident_bytes(h, n) == 192 * MiB);
    REQUIRE(seen_on && seen_off_after_on);
    return 0;
}

static int check_knob() {
    size_t n = (size_t)1 << 30;
    CopyWindow w;
    REQUIRE(copy_window_parse(nullptr, n, &w) && w.on && w.window == copy_window_rule(n).window);
    REQUIRE(copy_window_parse("", 4096, &w) && !w.on);
    REQUIRE(copy_window_parse("0", n, &w) && !w.on);
    REQUIRE(copy_window_parse("8192:0", n, &w) && w.on && w.unit == 1 && w.period == 2 && w.window == 0);
    REQUIRE(copy_window_parse("8192:8192", n, &w) && w.on && w.period == 2 && w.window == 2);
    REQUIRE(copy_window_parse("8192:4096", n, &w) && w.on && w.period == 2 && w.window == 1);
    REQUIRE(copy_window_parse("65536:12288", n, &w) && w.on && w.unit == 1 && w.period == 16 && w.window == 3);
    REQUIRE(copy_window_parse("65536:12288:8192", n, &w) && w.on && w.unit == 2 && w.period == 16 && w.window == 3);
    // the rule's own choice at 1 GiB: 1 MiB units, 32 to a period, 6 kept (period and window count units)
    REQUIRE(copy_window_parse("131072:24576:1048576", n, &w) && w.unit == 256 && w.period == 32 && w.window == 6);
    const char* bad[] = {"1", "4096", "x", "8192", "8192:", ":4096", "8192:4097", "8191:4096", "8192:12288", "12288:4096",
                         "0:0", "8192:4096:0", "8192:4096:12288", "8192:4096:4097", "8192:4096:4096:4096", "8192:4096:",
                         "8192;4096", "-8192:4096", " 8192:4096", "8192:4096 ", "0x2000:0x1000", "8192:4096:4096:",
                         "99999999999999999999999:4096", "17592186044416:4096"};
    for (const char* b : bad) {
        w.on = true;
        if (copy_window_parse(b, n, &w) || w.on) {
            fprintf(stderr, "MPX_COPY_WINDOW=\"%s\" was accepted\n", b);
            return 1;
        }
    }
    return 0;
}

int main() {
    if (check_rule() || check_knob()) return 1;
    printf("copy_window_host_check: ok\n");
    return 0;
}
