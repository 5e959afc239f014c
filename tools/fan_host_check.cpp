// fan_host_check — the host arithmetic of the fan exchange, as a stand-alone
// program for the host sanitizers (tools/asan_fan.sh builds it with
// -fsanitize=address,undefined and runs it once; no GPU, no libmpx):
//   * fan_default_nwg / link_nwg / fan_build_map (mpx_internal.h): what
//     mpx_xfer_fan builds its link table's widths and workgroup map with, and
//     link_nwg as the pair call's width rule too (prepare_call);
//   * mpxh_fan_stride / mpxh_fan_bytes / mpxh_fan_peers (mpx_host.c): the
//     block layout and peer lists of mpx_perf -m 1, and its -m validation.
// Every property is checked against a restatement written here; the first
// mismatch prints and exits 1.
#include "mpx_internal.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

extern "C" {
#include "mpx_host.h"
}

using namespace mpx;

#define REQUIRE(cond)                                                        \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: %s is false\n", __FILE__, __LINE__, #cond); \
            return 1;                                                        \
        }                                                                    \
    } while (0)

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static unsigned rnd(unsigned n) {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)(rng_state >> 33) % n;
}

static int check_widths() {
    const long long sizes[] = {0, 1, 15, 16, 17, 1023, 1024, 1025, 4097, 16384, 16385, 65555, 98305, 456131,
                               1 << 20, 4 << 20, 0x7fffffff};
    for (int nranks = 2; nranks <= MPX_MAX_RANKS; ++nranks)
        for (long long n : sizes)
            for (int same = 0; same <= 1; ++same) {
                const int w = fan_default_nwg(n, same != 0, nranks);
                const int cap = 128 / (nranks - 1) > 1 ? 128 / (nranks - 1) : 1;
                REQUIRE(w >= 1 && w <= cap && w <= bulk_nwg(n, same != 0));
                REQUIRE(w == cap || w == bulk_nwg(n, same != 0));
                const int nw = link_nwg(0, 0, w, n);
                REQUIRE(nw >= 1 && nw <= w);
                REQUIRE(nw == 1 || (long long)(nw - 1) * kMinPushChunk < n);   // every workgroup but the last: >= 1 KiB
                // the default grid of a rank with every peer stays resident with its peers'
                REQUIRE((long long)nw * (nranks - 1) <= 128);
            }
    REQUIRE(link_nwg(96, 0, 1, 98305) == 96 && link_nwg(0, 256, 1, 0) == 1 && link_nwg(200, 7, 1, 262144) == 200);
    return 0;
}

// The pair rule (prepare_call): the call's option, else MPX_PUSH_WG, else
// bulk_nwg; more than kMaxPushWG is refused; then at most one workgroup per
// kMinPushChunk bytes and at least one — restated here step by step, to hold
// the shared link_nwg against.
static int pair_width(int opt, int env, long long len, bool same) {
    long long w = opt > 0 ? opt : env > 0 ? env : bulk_nwg(len, same);
    if (w > kMaxPushWG) return 0;
    const long long most = (len + kMinPushChunk - 1) / kMinPushChunk;
    if (w > most) w = most;
    if (w < 1) w = 1;
    return (int)w;
}

static int check_pair_widths() {
    const long long sizes[] = {0, 1, 15, 16, 17, 1023, 1024, 1025, 4097, 16384, 16385, 65555, 98305, 456131,
                               1 << 20, 4 << 20, 0x7fffffff};
    const int widths[] = {-1, 0, 1, 2, 7, 64, 128, 255, 256, 257, 4096, 0x7fffffff};
    for (long long n : sizes)
        for (int same = 0; same <= 1; ++same)
            for (int opt : widths)
                for (int env : widths) {
                    const int w = link_nwg(opt, env, bulk_nwg(n, same != 0), n);
                    REQUIRE(w == pair_width(opt, env, n, same != 0));
                    const int chosen = opt > 0 ? opt : env > 0 ? env : bulk_nwg(n, same != 0);
                    REQUIRE((w == 0) == (chosen > kMaxPushWG));           // refused, never narrowed, above 256
                    REQUIRE(w == 0 || (w >= 1 && w <= chosen && w <= kMaxPushWG));
                    REQUIRE(w <= 1 || (long long)(w - 1) * kMinPushChunk < n);
                }
    // the size rule alone is never narrowed above 16 KiB (its chunks are 16-32 KiB)
    REQUIRE(link_nwg(0, 0, bulk_nwg(456131, true), 456131) == 28 && link_nwg(0, 0, bulk_nwg(456131, false), 456131) == 14);
    REQUIRE(link_nwg(0, 0, bulk_nwg(4 << 20, true), 4 << 20) == 128 && link_nwg(64, 0, 128, 4097) == 5);
    return 0;
}

static int check_map() {
    auto tab = std::make_unique<FanTable>();
    for (int round = 0; round < 2000; ++round) {
        const int nlinks = 1 + (int)rnd(MPX_MAX_RANKS - 1);
        int nwg[MPX_MAX_RANKS];
        long long sum = 0;
        for (int k = 0; k < nlinks; ++k) sum += nwg[k] = 1 + (int)rnd(round % 3 == 0 ? 256 : 8);
        const int iters = (int)rnd(1000);
        memset(tab.get(), 0xff, sizeof(FanTable));
        const int grid = fan_build_map(tab.get(), nlinks, nwg, iters);
        if (sum > kFanMaxGrid) {
            REQUIRE(grid == -1);
            continue;
        }
        REQUIRE(grid == (int)sum);
        // every (link, workgroup) exactly once; workgroup w of every link before w + 1 of any
        static unsigned char seen[MPX_MAX_RANKS][kMaxPushWG];
        memset(seen, 0, sizeof seen);
        int last_w = 0;
        for (int b = 0; b < grid; ++b) {
            const int k = (int)(tab->map[b] >> 16), w = (int)(tab->map[b] & 0xffffu);
            REQUIRE(k < nlinks && w < nwg[k] && !seen[k][w]);
            seen[k][w] = 1;
            REQUIRE(w >= last_w);
            last_w = w;
        }
        for (int b = grid; b < kFanMaxGrid; ++b) REQUIRE(tab->map[b] == 0xffffffffu);   // nothing past the grid
        for (int k = 0; k < nlinks; ++k) REQUIRE(tab->link[k].nwg == nwg[k] && tab->link[k].csum0 == k * iters);
    }
    int bad[2] = {0, 3};
    REQUIRE(fan_build_map(tab.get(), 2, bad, 1) == -1);
    bad[0] = 257;
    REQUIRE(fan_build_map(tab.get(), 2, bad, 1) == -1);
    REQUIRE(fan_build_map(tab.get(), 0, bad, 1) == -1 && fan_build_map(tab.get(), MPX_MAX_RANKS + 1, bad, 1) == -1);
    return 0;
}

static int check_host() {
    REQUIRE(mpxh_fan_stride(0) == 0 && mpxh_fan_stride(1) == 4096 && mpxh_fan_stride(4096) == 4096);
    REQUIRE(mpxh_fan_stride(4097) == 8192 && mpxh_fan_stride(65555) == 69632 && mpxh_fan_stride(-1) == 0);
    REQUIRE(mpxh_fan_stride(0x7fffffff) == 0x80000000ull);
    REQUIRE(mpxh_fan_bytes(3, 65555) == 3 * 69632 && mpxh_fan_bytes(8, 4 << 20) == (size_t)32 << 20);
    REQUIRE(mpxh_fan_bytes(64, 32 << 20) == 0 && mpxh_fan_bytes(2, 0x7fffffff) == 0 && mpxh_fan_bytes(0, 8) == 0);
    for (int world = 2; world <= MPXH_MAX_RANKS; ++world)
        for (int r = 0; r < world; ++r) {
            int peers[MPXH_MAX_RANKS];
            REQUIRE(mpxh_fan_peers(world, r, peers) == world - 1);
            for (int k = 0; k < world - 1; ++k) REQUIRE(peers[k] == (k < r ? k : k + 1));
        }
    // the -m rules of mpxh_validate, each with its own message
    FILE* sink = tmpfile();
    REQUIRE(sink != nullptr);
    mpxh_options o;
    auto fresh = [&] {
        mpxh_defaults(&o);
        o.fan = 1;
        o.group_size = 1;
        o.ppn = 1;
        o.buff_sz = 65555;
    };
    fresh();
    REQUIRE(mpxh_validate(&o, 3, sink) == 0);
    fresh(); o.all_pairs = 1;            REQUIRE(mpxh_validate(&o, 4, sink) == 1);
    fresh(); o.arm_set = 1;              REQUIRE(mpxh_validate(&o, 3, sink) == 1);
    fresh(); o.arm_set = 1; o.arm = 0;   REQUIRE(mpxh_validate(&o, 3, sink) == 0);
    fresh(); o.lat_cap = 0;              REQUIRE(mpxh_validate(&o, 3, sink) == 1);
    fresh(); o.engine = 1;               REQUIRE(mpxh_validate(&o, 3, sink) == 1);
    fresh(); o.use_dotnet = 1;           REQUIRE(mpxh_validate(&o, 3, sink) == 1);
    fresh(); o.buff_sz = 0x7fffffff;     REQUIRE(mpxh_validate(&o, 3, sink) == 1);
    fresh(); o.sweep_min = 1; o.sweep_max = 1 << 30; REQUIRE(mpxh_validate(&o, 3, sink) == 1);
    // -P (the link recorder) goes with -m 2 only
    fresh(); o.fan_lat_cap = 64;                            REQUIRE(mpxh_validate(&o, 3, sink) == 1);
    fresh(); o.fan = 2; o.buff_sz = 4096; o.fan_lat_cap = 64; REQUIRE(mpxh_validate(&o, 3, sink) == 0);
    fresh(); o.fan = 0; o.fan_lat_cap = 0;                  REQUIRE(mpxh_validate(&o, 2, sink) == 1);
    fresh(); o.fan = 2; o.buff_sz = 8; o.fan_lat_cap = 0; o.lat_cap = 0; REQUIRE(mpxh_validate(&o, 3, sink) == 1);
    {
        const char* argv[] = {"x", "-m", "2", "-P", "65536", nullptr};
        mpxh_defaults(&o);
        REQUIRE(o.fan_lat_cap == -1);
        REQUIRE(mpxh_parse_args(&o, 5, const_cast<char**>(argv)) == MPXH_PARSE_OK && o.fan_lat_cap == 65536 && o.fan == 2);
        for (const char* bad : {"-1", "x", "12x", "65537"}) {
            const char* av[] = {"x", "-P", bad, nullptr};
            mpxh_defaults(&o);
            REQUIRE(mpxh_parse_args(&o, 3, const_cast<char**>(av)) == MPXH_PARSE_BAD_VALUE);
        }
    }
    fclose(sink);
    return 0;
}

int main() {
    if (check_widths() || check_pair_widths() || check_map() || check_host()) return 1;
    puts("fan_host_check: ok");
    return 0;
}
