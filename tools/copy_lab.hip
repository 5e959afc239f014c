// copy_lab.hip — standalone tuning lab for the HBM copy kernel (not product
// code; the product kernel is k_copy in mpi-perf_amd/csrc/mpx_kernels.hip).
// Times every variant over a 1 GiB copy with HIP events (avg of 20 launches,
// best of 5 reps) and checks the output.  One JSON line per variant.
//   hipcc --offload-arch=gfx950 -O3 -o tools/copy_lab tools/copy_lab.hip
//   tools/copy_lab <bytes> [filter [dst_off src_off]]    the variant table
//   tools/copy_lab <bytes> win|win2 [filter [filter]]    the window lab (below)
//   tools/copy_lab <bytes> pol [filter [windows]]        cache policies of the window form's streamed side
//   tools/copy_lab <bytes> keep [filter [windows [K [J [all|kept]]]]]   how much of the window is resident
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

typedef unsigned int v4u __attribute__((ext_vector_type(4)));
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e)); exit(1); } } while (0)

constexpr unsigned kW3 = 0x00020000;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const void* base, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, kW3);
}

// A: block-contiguous chunk, plain/nt pointer loads (product form)
template <int T, int U, bool NT>
__global__ __launch_bounds__(T) void kA(const v4u* __restrict__ s, v4u* __restrict__ d, size_t n16) {
    const size_t per = (n16 + gridDim.x - 1) / gridDim.x;
    const size_t lo = (size_t)blockIdx.x * per;
    const size_t end = lo + per < n16 ? lo + per : n16;
    size_t i = lo + threadIdx.x;
    for (; i + (U - 1) * T < end; i += U * T) {
        v4u r[U];
#pragma unroll
        for (int u = 0; u < U; ++u) r[u] = NT ? __builtin_nontemporal_load(s + i + u * T) : s[i + u * T];
#pragma unroll
        for (int u = 0; u < U; ++u) { if (NT) __builtin_nontemporal_store(r[u], d + i + u * T); else d[i + u * T] = r[u]; }
    }
    for (; i < end; i += T) d[i] = s[i];
}

// B: block-contiguous chunk with buffer ops and explicit cache-policy aux
template <int T, int U, int LA, int SA>
__global__ __launch_bounds__(T) void kB(const unsigned char* s, unsigned char* d, size_t n, size_t per) {
    const size_t lo = (size_t)blockIdx.x * per;
    if (lo >= n) return;
    const unsigned bytes = (unsigned)(lo + per < n ? per : n - lo);
    const __amdgpu_buffer_rsrc_t rs = rsrc(s + lo, bytes), rd = rsrc(d + lo, bytes);
    unsigned o = threadIdx.x * 16;
    for (; o + (U - 1) * T * 16 < bytes; o += U * T * 16) {
        v4u r[U];
#pragma unroll
        for (int u = 0; u < U; ++u) r[u] = __builtin_amdgcn_raw_buffer_load_b128(rs, o + u * T * 16, 0, LA);
#pragma unroll
        for (int u = 0; u < U; ++u) __builtin_amdgcn_raw_buffer_store_b128(r[u], rd, o + u * T * 16, 0, SA);
    }
    for (; o < bytes; o += T * 16)
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_amdgcn_raw_buffer_load_b128(rs, o, 0, LA), rd, o, 0, SA);
}

// C: wave tiles — each wave copies a contiguous (U KiB) tile per step, tiles
// assigned grid-stride over all waves (DRAM-page-friendly, no block chunk)
template <int T, int U, bool NT>
__global__ __launch_bounds__(T) void kC(const v4u* __restrict__ s, v4u* __restrict__ d, size_t n16) {
    const size_t waves = (size_t)gridDim.x * (T / 64);
    const size_t w = (size_t)blockIdx.x * (T / 64) + (threadIdx.x >> 6);
    const unsigned lane = threadIdx.x & 63;
    const size_t tile = 64 * U;   // 16-B units per wave tile
    for (size_t t = w * tile; t < n16; t += waves * tile) {
        v4u r[U];
        if (t + tile <= n16) {
#pragma unroll
            for (int u = 0; u < U; ++u) r[u] = NT ? __builtin_nontemporal_load(s + t + u * 64 + lane) : s[t + u * 64 + lane];
#pragma unroll
            for (int u = 0; u < U; ++u) { if (NT) __builtin_nontemporal_store(r[u], d + t + u * 64 + lane); else d[t + u * 64 + lane] = r[u]; }
        } else {
            for (size_t i = t + lane; i < n16; i += 64) d[i] = s[i];
        }
    }
}

// D: persistent block-contiguous, XCD-aware: blocks b, b+8, b+16.. run on one
// XCD; give each XCD one contiguous eighth of the buffer
template <int T, int U>
__global__ __launch_bounds__(T) void kD(const v4u* __restrict__ s, v4u* __restrict__ d, size_t n16) {
    const unsigned G = gridDim.x, b = blockIdx.x;
    const unsigned xcd = b & 7, k = b >> 3, per_xcd = G >> 3;
    const unsigned vb = xcd * per_xcd + k;       // virtual block: contiguous per XCD
    const size_t per = (n16 + G - 1) / G;
    const size_t lo = (size_t)vb * per;
    const size_t end = lo + per < n16 ? lo + per : n16;
    size_t i = lo + threadIdx.x;
    for (; i + (U - 1) * T < end; i += U * T) {
        v4u r[U];
#pragma unroll
        for (int u = 0; u < U; ++u) r[u] = __builtin_nontemporal_load(s + i + u * T);
#pragma unroll
        for (int u = 0; u < U; ++u) __builtin_nontemporal_store(r[u], d + i + u * T);
    }
    for (; i < end; i += T) d[i] = s[i];
}


// E: one step per block, no loop: block b copies units [b*T*U, (b+1)*T*U)
template <int T, int U>
__global__ __launch_bounds__(T) void kE(const v4u* __restrict__ s, v4u* __restrict__ d, size_t n16) {
    const size_t base = (size_t)blockIdx.x * (T * U) + threadIdx.x;
    if (base + (U - 1) * T < n16) {
        v4u r[U];
#pragma unroll
        for (int u = 0; u < U; ++u) r[u] = __builtin_nontemporal_load(s + base + u * T);
#pragma unroll
        for (int u = 0; u < U; ++u) __builtin_nontemporal_store(r[u], d + base + u * T);
    } else {
        for (size_t i = base; i < n16; i += T) d[i] = s[i];
    }
}
template <int T, int U> void runE(const void* s, void* d, size_t n, int, int, hipStream_t st) {
    const size_t n16 = n / 16, g = (n16 + T * U - 1) / (T * U);
    hipLaunchKernelGGL((kE<T, U>), dim3((unsigned)g), dim3(T), 0, st, (const v4u*)s, (v4u*)d, n16);
}
// R / W: one-direction ceilings of the same shape (one 16-B unit per lane,
// one step per workgroup): R reads src (nontemporal) and folds it into one
// word per workgroup; W stores a constant.  Timed traffic is B per launch;
// the lab's rate column counts 2B, so halve it for these two.
__global__ __launch_bounds__(256) void kR(const v4u* __restrict__ s, v4u* __restrict__ d, size_t n16) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    v4u r = {0, 0, 0, 0};
    if (i < n16) r = __builtin_nontemporal_load(s + i);
    unsigned x = r.x ^ r.y ^ r.z ^ r.w;
    for (int o = 32; o > 0; o >>= 1) x ^= __shfl_xor(x, o);
    if (x == 0x9e3779b9u && threadIdx.x == 0) d[blockIdx.x] = r;   // keeps the loads live
}
__global__ __launch_bounds__(256) void kW(const v4u* __restrict__, v4u* __restrict__ d, size_t n16) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const v4u v = {(unsigned)i, 1u, 2u, 3u};
    if (i < n16) __builtin_nontemporal_store(v, d + i);
}
void runR(const void* s, void* d, size_t n, int, int, hipStream_t st) {
    hipLaunchKernelGGL(kR, dim3((unsigned)((n / 16 + 255) / 256)), dim3(256), 0, st, (const v4u*)s, (v4u*)d, n / 16);
}
void runW(const void* s, void* d, size_t n, int, int, hipStream_t st) {
    hipLaunchKernelGGL(kW, dim3((unsigned)((n / 16 + 255) / 256)), dim3(256), 0, st, (const v4u*)s, (v4u*)d, n / 16);
}
// M: the runtime's own device-to-device copy
void runM(const void* s, void* d, size_t n, int, int, hipStream_t st) { (void)hipMemcpyAsync(d, s, n, hipMemcpyDeviceToDevice, st); }

__global__ void kfill(unsigned* p, size_t n4) {
    for (size_t i = blockIdx.x * 256ull + threadIdx.x; i < n4; i += gridDim.x * 256ull) p[i] = (unsigned)(i * 2654435761u) ^ 0x5a5a1234u;
}
__global__ void kcmp(const unsigned* a, const unsigned* b, size_t n4, unsigned* bad) {
    for (size_t i = blockIdx.x * 256ull + threadIdx.x; i < n4; i += gridDim.x * 256ull)
        if (a[i] != b[i]) atomicAdd(bad, 1u);
}

struct Var { const char* name; int grid, threads; void (*run)(const void*, void*, size_t, int, int, hipStream_t); };

template <int T, int U, bool NT> void runA(const void* s, void* d, size_t n, int g, int, hipStream_t st) {
    hipLaunchKernelGGL((kA<T, U, NT>), dim3(g), dim3(T), 0, st, (const v4u*)s, (v4u*)d, n / 16);
}
template <int T, int U, int LA, int SA> void runB(const void* s, void* d, size_t n, int g, int, hipStream_t st) {
    size_t per = ((n + g - 1) / g + 15) & ~(size_t)15;
    hipLaunchKernelGGL((kB<T, U, LA, SA>), dim3(g), dim3(T), 0, st, (const unsigned char*)s, (unsigned char*)d, n, per);
}
template <int T, int U, bool NT> void runC(const void* s, void* d, size_t n, int g, int, hipStream_t st) {
    hipLaunchKernelGGL((kC<T, U, NT>), dim3(g), dim3(T), 0, st, (const v4u*)s, (v4u*)d, n / 16);
}
template <int T, int U> void runD(const void* s, void* d, size_t n, int g, int, hipStream_t st) {
    hipLaunchKernelGGL((kD<T, U>), dim3(g), dim3(T), 0, st, (const v4u*)s, (v4u*)d, n / 16);
}

// ---------------------------------------------------------------------------
// Window lab (`copy_lab <bytes> win [filter]`): can a striped subset of a
// repeatedly copied buffer stay in the 256 MiB Infinity Cache while the rest
// streams past it?  The shipped shape (one 16-B unit per lane, one step per
// workgroup) with the cache policy picked per workgroup: 4 KiB block b is
// "kept" when (b / unit) % period < window (unit in blocks, period and window
// in units; unit and period are powers of two, so the test is a shift, a mask
// and a compare on the scalar unit).  Kept blocks use aux LA on the load (LW)
// and / or default-policy stores (SW); every other access is nontemporal.
// The branch is uniform and the two buffer loads carry different constant
// aux, so they cannot be merged.  Results: profiles/copy_window_lab.jsonl.
struct Win { unsigned unit_shift, period_mask, window; };
template <int LA, bool LW, bool SW>
__global__ __launch_bounds__(256) void kWin(const unsigned char* s, unsigned char* d, size_t n, Win w) {
    const size_t lo = (size_t)blockIdx.x * 4096;
    const unsigned bytes = n - lo < 4096 ? (unsigned)(n - lo) & ~15u : 4096u;   // the buffer bounds the last block
    const __amdgpu_buffer_rsrc_t rs = rsrc(s + lo, bytes), rd = rsrc(d + lo, bytes);
    const unsigned o = threadIdx.x * 16;
    if (((blockIdx.x >> w.unit_shift) & w.period_mask) < w.window) {
        const v4u r = __builtin_amdgcn_raw_buffer_load_b128(rs, o, 0, LW ? LA : 2);
        __builtin_amdgcn_raw_buffer_store_b128(r, rd, o, 0, SW ? 0 : 2);
    } else {
        const v4u r = __builtin_amdgcn_raw_buffer_load_b128(rs, o, 0, 2);
        __builtin_amdgcn_raw_buffer_store_b128(r, rd, o, 0, 2);
    }
}
// The same with the shipped instructions on every block that is not kept: a
// nontemporal pointer load and store, as kE<256, 1>.  Only a kept block goes
// through a buffer descriptor (default policy).  A pointer load and a buffer
// load cannot be merged either, and the streamed blocks pay nothing for the
// descriptor (`copy_lab <bytes> win2`).
template <bool LW, bool SW>
__global__ __launch_bounds__(256) void kWinP(const unsigned char* s, unsigned char* d, size_t n, Win w) {
    const size_t n16 = n / 16, i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const v4u* sp = (const v4u*)s;
    v4u* dp = (v4u*)d;
    if (((blockIdx.x >> w.unit_shift) & w.period_mask) < w.window) {
        const size_t lo = (size_t)blockIdx.x * 4096;
        const unsigned bytes = n - lo < 4096 ? (unsigned)(n - lo) & ~15u : 4096u;
        const unsigned o = threadIdx.x * 16;
        v4u r;
        if (LW) r = __builtin_amdgcn_raw_buffer_load_b128(rsrc(s + lo, bytes), o, 0, 0);
        else if (i < n16) r = __builtin_nontemporal_load(sp + i);
        if (SW) __builtin_amdgcn_raw_buffer_store_b128(r, rsrc(d + lo, bytes), o, 0, 0);
        else if (i < n16) __builtin_nontemporal_store(r, dp + i);
    } else if (i < n16) {
        __builtin_nontemporal_store(__builtin_nontemporal_load(sp + i), dp + i);
    }
}
typedef void (*WinKernel)(const unsigned char*, unsigned char*, size_t, Win);
struct WinVar { char name[48]; WinKernel k; Win w; };   // k == nullptr: the shipped form, E_t256_u1
static void win_run(const WinVar& v, const void* s, void* d, size_t n, hipStream_t st) {
    if (!v.k) return runE<256, 1>(s, d, n, 0, 0, st);
    hipLaunchKernelGGL(v.k, dim3((unsigned)((n + 4095) / 4096)), dim3(256), 0, st, (const unsigned char*)s,
                       (unsigned char*)d, n, v.w);
}
struct WinTimes { double one, many, fresh; };   // us per copy
// One repetition of one form: a single timed copy after a priming one, 20
// copies behind one start, and the no-reuse control: `pairs` buffer pairs in
// rotation (3 at 1 GiB), so a line returns only after 2 * pairs * n bytes.
static WinTimes win_measure(const WinVar& v, char* const* s, char* const* d, int pairs, size_t n, hipStream_t st,
                            hipEvent_t e0, hipEvent_t e1) {
    WinTimes t;
    float ms;
    win_run(v, s[0], d[0], n, st);
    CK(hipEventRecord(e0, st));
    win_run(v, s[0], d[0], n, st);
    CK(hipEventRecord(e1, st));
    CK(hipEventSynchronize(e1));
    CK(hipEventElapsedTime(&ms, e0, e1));
    t.one = ms * 1e3;
    CK(hipEventRecord(e0, st));
    for (int l = 0; l < 20; ++l) win_run(v, s[0], d[0], n, st);
    CK(hipEventRecord(e1, st));
    CK(hipEventSynchronize(e1));
    CK(hipEventElapsedTime(&ms, e0, e1));
    t.many = ms * 1e3 / 20;
    for (int p = 0; p < pairs; ++p) win_run(v, s[p], d[p], n, st);
    CK(hipEventRecord(e0, st));
    for (int l = 0; l < 2 * pairs; ++l) win_run(v, s[l % pairs], d[l % pairs], n, st);
    CK(hipEventRecord(e1, st));
    CK(hipEventSynchronize(e1));
    CK(hipEventElapsedTime(&ms, e0, e1));
    t.fresh = ms * 1e3 / (2 * pairs);
    CK(hipGetLastError());
    return t;
}
static void win_stats(const double* x, int k, double* lo, double* med, double* hi) {
    std::vector<double> v(x, x + k);
    for (int i = 0; i < k; ++i) for (int j = i + 1; j < k; ++j) if (v[j] < v[i]) { double t = v[i]; v[i] = v[j]; v[j] = t; }
    *lo = v[0], *med = v[k / 2], *hi = v[k - 1];
}
constexpr int kReps = 5;
// One form against another (`base`) in one process: the output check, kReps
// alternating repetitions of win_measure, and one JSON line holding every
// repetition of both with the two conditions.
static void win_ab(const WinVar& v, const WinVar& base, char* const* s, char* const* d, int pairs, size_t n,
                   unsigned* bad, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
    CK(hipMemsetAsync(d[0], 0, n, st));
    win_run(v, s[0], d[0], n, st);
    CK(hipGetLastError());
    CK(hipMemsetAsync(bad, 0, 4, st));
    hipLaunchKernelGGL(kcmp, dim3(4096), dim3(256), 0, st, (const unsigned*)s[0], (const unsigned*)d[0], n / 4, bad);
    unsigned nb = 0;
    CK(hipMemcpyAsync(&nb, bad, 4, hipMemcpyDeviceToHost, st));
    CK(hipStreamSynchronize(st));
    double t[2][3][kReps];   // [base, variant][one, many, fresh][rep]
    for (int rep = 0; rep < kReps; ++rep)
        for (int side = 0; side < 2; ++side) {
            const WinTimes x = win_measure(side ? v : base, s, d, pairs, n, st, e0, e1);
            t[side][0][rep] = x.one, t[side][1][rep] = x.many, t[side][2][rep] = x.fresh;
        }
    // the two conditions: slowest repetition of the variant under the base
    // form's fastest with reuse; no-reuse median not above the base form's
    // slowest
    double lo[2][3], med[2][3], hi[2][3];
    for (int side = 0; side < 2; ++side)
        for (int m = 0; m < 3; ++m) win_stats(t[side][m], kReps, &lo[side][m], &med[side][m], &hi[side][m]);
    // one line per form: every repetition of the three figures, the form's
    // and the base form's beside it (us per copy, in the order measured)
    printf("{\"variant\": \"%s\", \"base\": \"%s\", \"bytes\": %zu, \"unit_period_window\": [%u, %u, %u], \"noreuse_pairs\": %d",
           v.name, base.name, n, 1u << v.w.unit_shift, v.w.period_mask + 1, v.w.window, pairs);
    const char* keys[2][3] = {{"base_one", "base_x20", "base_noreuse"}, {"one", "x20", "noreuse"}};
    for (int side = 1; side >= 0; --side)
        for (int m = 0; m < 3; ++m) {
            printf(", \"%s\": [", keys[side][m]);
            for (int rep = 0; rep < kReps; ++rep) printf("%s%.1f", rep ? ", " : "", t[side][m][rep]);
            printf("]");
        }
    printf(", \"reuse_gain\": %s, \"noreuse_ok\": %s, \"bad_words\": %u}\n",
           hi[1][1] < lo[0][1] && hi[1][0] < lo[0][0] ? "true" : "false", med[1][2] <= hi[0][2] ? "true" : "false", nb);
    fflush(stdout);
}
static int win_lab(size_t n, const char* only, const char* also, bool second) {
    const size_t MiB = 1ull << 20;
    const int pairs = (int)((3ull << 30) / n) < 3 ? 3 : (int)((3ull << 30) / n);
    std::vector<char*> s(pairs), d(pairs);
    unsigned* bad;
    hipStream_t st;
    CK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    for (int p = 0; p < pairs; ++p) {
        CK(hipMalloc(&s[p], n));
        CK(hipMalloc(&d[p], n));
        hipLaunchKernelGGL(kfill, dim3(4096), dim3(256), 0, st, (unsigned*)s[p], n / 4);
    }
    CK(hipMalloc(&bad, 4));
    CK(hipStreamSynchronize(st));
    // W MiB resident out of n as window / 32 units of every period (both: the
    // same units of src and dst, W / 2 each, so 64 units to a period); a form
    // whose period does not fit n is left out.  aux: sc0 = 1, nt = 2, sc1 = 16
    struct Form { const char* tag; WinKernel k; bool both; };
    struct Unit { const char* name; size_t bytes; };
    const std::vector<Form> forms =
        !second ? std::vector<Form>{{"L0", kWin<0, true, false>, false}, {"L1", kWin<1, true, false>, false},
                                    {"L16", kWin<16, true, false>, false}, {"L17", kWin<17, true, false>, false},
                                    {"S", kWin<0, false, true>, false},      // the mirror image: a window of dst
                                    {"LS", kWin<0, true, true>, true}}
                : std::vector<Form>{{"PL", kWinP<true, false>, false}, {"PS", kWinP<false, true>, false},
                                    {"PLS", kWinP<true, true>, true}};
    // win2: finer units, and W up to past the cache's size
    const std::vector<Unit> units = !second ? std::vector<Unit>{{"64K", 64 << 10}, {"1M", 1 << 20}, {"16M", 16 << 20}}
                                            : std::vector<Unit>{{"64K", 64 << 10}, {"256K", 256 << 10}, {"1M", 1 << 20}, {"4M", 4 << 20}};
    const std::vector<size_t> Ws = !second ? std::vector<size_t>{64, 128, 160, 192, 224}
                                           : std::vector<size_t>{96, 128, 160, 192, 224, 256, 320};
    const WinVar base = {"E_t256_u1", nullptr, {0, 0, 0}};
    // first the form itself with no block kept
    std::vector<WinVar> vs = {second ? WinVar{"win_Pallnt", kWinP<true, false>, {0, 0, 0}}
                                     : WinVar{"win_allnt", kWin<0, true, false>, {0, 0, 0}}};
    for (const Form& f : forms)
        for (const Unit& u : units) {
            size_t lastW = 0;
            for (size_t W : Ws) {
                if (W * MiB > n) W = n / MiB;
                const unsigned period = f.both ? 64 : 32;
                if (W == lastW || u.bytes * period > n) continue;
                lastW = W;
                WinVar v;
                snprintf(v.name, sizeof v.name, "win_%s_W%zu_u%s", f.tag, W, u.name);
                v.k = f.k;
                v.w = {(unsigned)__builtin_ctzll(u.bytes / 4096), period - 1, (unsigned)(W * MiB * 32 / n)};
                vs.push_back(v);
            }
        }
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    for (int w = 0; w < 3; ++w) win_run(base, s[0], d[0], n, st);   // clocks up
    for (const WinVar& v : vs) {
        if ((only && !strstr(v.name, only)) || (also && !strstr(v.name, also))) continue;
        win_ab(v, base, s.data(), d.data(), pairs, n, bad, st, e0, e1);
    }
    return 0;
}

// ---------------------------------------------------------------------------
// Policy lab (`copy_lab <bytes> pol [filter [windows]]`): the product's form,
// kWinP<true, false>, with the cache policy of its STREAMED side as the
// parameter.  Kept blocks load through a descriptor with the default policy,
// as shipped; every other load carries LA and every store SA: kPtrNt is the
// shipped nontemporal pointer instruction, anything else the aux of a buffer
// op (sc0 = 1, nt = 2, sc1 = 16).  Each form alternates with the shipped form
// at the same window and is judged by win_ab's two conditions.
// `windows` is a comma-separated list of resident MiB (1 MiB units, 32 to a
// period, as `win2`) or of "period:window:unit" as MPX_COPY_WINDOW takes it.
constexpr int kPtrNt = -1;
template <int LA>
__device__ __forceinline__ v4u pol_load(const unsigned char* s, size_t n) {
    v4u r = {0, 0, 0, 0};
    if constexpr (LA == kPtrNt) {
        const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
        if (i < n / 16) r = __builtin_nontemporal_load((const v4u*)s + i);
    } else {
        const size_t lo = (size_t)blockIdx.x * 4096;
        const unsigned bytes = n - lo < 4096 ? (unsigned)(n - lo) & ~15u : 4096u;
        r = __builtin_amdgcn_raw_buffer_load_b128(rsrc(s + lo, bytes), threadIdx.x * 16, 0, LA);
    }
    return r;
}
template <int SA>
__device__ __forceinline__ void pol_store(unsigned char* d, size_t n, v4u r) {
    if constexpr (SA == kPtrNt) {
        const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
        if (i < n / 16) __builtin_nontemporal_store(r, (v4u*)d + i);
    } else {
        const size_t lo = (size_t)blockIdx.x * 4096;
        const unsigned bytes = n - lo < 4096 ? (unsigned)(n - lo) & ~15u : 4096u;
        __builtin_amdgcn_raw_buffer_store_b128(r, rsrc(d + lo, bytes), threadIdx.x * 16, 0, SA);
    }
}
__device__ __forceinline__ bool win_kept(Win w) { return ((blockIdx.x >> w.unit_shift) & w.period_mask) < w.window; }
// grid = ceil(n / 4096) for the three of them, so every workgroup's block starts inside the buffer
template <int LA, int SA>
__global__ __launch_bounds__(256) void kPol(const unsigned char* s, unsigned char* d, size_t n, Win w) {
    v4u r;
    if (win_kept(w)) r = pol_load<0>(s, n);
    else r = pol_load<LA>(s, n);
    pol_store<SA>(d, n, r);
}
// The copy's halves, each alone: the streamed loads of the un-kept blocks of
// src with the result folded away (a kept block's workgroup does nothing),
// and the stores of dst (a constant).  sink holds one unit per workgroup.
template <int LA>
__global__ __launch_bounds__(256) void kHalfL(const unsigned char* s, unsigned char* sink, size_t n, Win w) {
    if (win_kept(w)) return;
    const v4u r = pol_load<LA>(s, n);
    unsigned x = r.x ^ r.y ^ r.z ^ r.w;
    for (int o = 32; o > 0; o >>= 1) x ^= __shfl_xor(x, o);
    if (x == 0x9e3779b9u && threadIdx.x == 0) ((v4u*)sink)[blockIdx.x] = r;   // keeps the loads live
}
template <int SA>
__global__ __launch_bounds__(256) void kHalfS(const unsigned char*, unsigned char* d, size_t n, Win) {
    const v4u v = {blockIdx.x, threadIdx.x, 2u, 3u};
    pol_store<SA>(d, n, v);
}
struct Pol { const char *ln, *sn; WinKernel copy, loads, stores; };
#define POL_ROW(LA, LN) \
    {LN, "p", kPol<LA, kPtrNt>, kHalfL<LA>, kHalfS<kPtrNt>}, {LN, "nt", kPol<LA, 2>, kHalfL<LA>, kHalfS<2>}, \
    {LN, "sc1", kPol<LA, 16>, kHalfL<LA>, kHalfS<16>}, {LN, "sc1nt", kPol<LA, 18>, kHalfL<LA>, kHalfS<18>}, \
    {LN, "sys", kPol<LA, 17>, kHalfL<LA>, kHalfS<17>}, {LN, "sysnt", kPol<LA, 19>, kHalfL<LA>, kHalfS<19>}
// the first is the shipped form written this way (a control: it must tie)
static const Pol kPols[] = {POL_ROW(kPtrNt, "p"), POL_ROW(2, "nt"), POL_ROW(16, "sc1"),
                            POL_ROW(18, "sc1nt"), POL_ROW(17, "sys"), POL_ROW(19, "sysnt")};
static void pol_name(const Pol& p, const Win& w, size_t n, char* out, size_t cap) {
    const size_t res = (size_t)w.window * (4096ull << w.unit_shift) *
                       ((n + (4096ull << w.unit_shift) * (w.period_mask + 1) - 1) / ((4096ull << w.unit_shift) * (w.period_mask + 1)));
    snprintf(out, cap, "pol_L%s_S%s_W%zu", p.ln, p.sn, res >> 20);
}
// "192" (MiB resident: 1 MiB units, 32 to a period) or "period:window:unit"
static bool win_spec(const char* v, size_t n, Win* w) {
    unsigned long long f[3] = {0, 0, 4096};
    const int k = sscanf(v, "%llu:%llu:%llu", &f[0], &f[1], &f[2]);
    if (k == 1) {
        const unsigned long long win = f[0] * (1ull << 20) * 32 / n;
        if (win > 32 || (32ull << 20) > n) return false;
        *w = {8, 31, (unsigned)win};
        return true;
    }
    if (k < 2 || f[0] % 4096 || f[1] % 4096 || f[2] % 4096 || !f[0] || !f[2] || f[1] > f[0]) return false;
    const unsigned long long period = f[0] / 4096, unit = f[2] / 4096;
    if ((period & (period - 1)) || (unit & (unit - 1))) return false;
    *w = {(unsigned)__builtin_ctzll(unit), (unsigned)period - 1, (unsigned)(f[1] / 4096)};
    return true;
}
static std::vector<Win> win_specs(const char* list, size_t n) {
    std::vector<Win> ws;
    char buf[256];
    snprintf(buf, sizeof buf, "%s", list && *list ? list : "192");
    for (char* tok = strtok(buf, ","); tok; tok = strtok(nullptr, ",")) {
        Win w;
        if (!win_spec(tok, n, &w)) { fprintf(stderr, "window '%s' does not fit %zu bytes\n", tok, n); exit(2); }
        ws.push_back(w);
    }
    return ws;
}
struct Lab {
    int pairs;
    std::vector<char*> s, d;
    unsigned char* sink;
    unsigned* bad;
    hipStream_t st;
    hipEvent_t e0, e1;
};
static Lab lab_open(size_t n) {
    Lab L;
    L.pairs = (int)((3ull << 30) / n) < 3 ? 3 : (int)((3ull << 30) / n);
    L.s.resize(L.pairs), L.d.resize(L.pairs);
    CK(hipStreamCreateWithFlags(&L.st, hipStreamNonBlocking));
    for (int p = 0; p < L.pairs; ++p) {
        CK(hipMalloc(&L.s[p], n));
        CK(hipMalloc(&L.d[p], n));
        hipLaunchKernelGGL(kfill, dim3(4096), dim3(256), 0, L.st, (unsigned*)L.s[p], n / 4);
    }
    CK(hipMalloc(&L.sink, (n + 4095) / 4096 * 16));   // one unit per workgroup of any grid here
    CK(hipMalloc(&L.bad, 4));
    CK(hipEventCreate(&L.e0));
    CK(hipEventCreate(&L.e1));
    CK(hipStreamSynchronize(L.st));
    return L;
}
static int pol_lab(size_t n, const char* only, const char* windows) {
    Lab L = lab_open(n);
    for (const Win& w : win_specs(windows, n)) {
        WinVar base = {"", kWinP<true, false>, w};
        snprintf(base.name, sizeof base.name, "win_PL");
        for (int k = 0; k < 3; ++k) win_run(base, L.s[0], L.d[0], n, L.st);   // clocks up
        for (const Pol& p : kPols) {
            WinVar v = {"", p.copy, w};
            pol_name(p, w, n, v.name, sizeof v.name);
            if (only && !strstr(v.name, only)) continue;
            win_ab(v, base, L.s.data(), L.d.data(), L.pairs, n, L.bad, L.st, L.e0, L.e1);
        }
    }
    return 0;
}

// ---------------------------------------------------------------------------
// Residency probe (`copy_lab <bytes> keep [filter [windows [K [J [which]]]]]`):
// how much of the window is in the Infinity Cache when the next copy comes to
// read it?  The probe is a read-only pass in R_read_only's shape over a
// selection of src's blocks: `window` units from unit `first` of every whole
// period, i.e. the kept blocks (first = 0) or as many streamed ones at the
// same stripe geometry (first = period / 2).  Per repetition three timed
// passes over the same selection of s[0]:
//   hit    right after two default-policy reads of just that selection
//   miss   after the flush: the form's copies over every other buffer pair,
//          twice (the no-reuse rotation), then a default-policy read of the
//          whole of s[1]
//   case   after the flush, K copies s[0] -> d[0] with the form under test
//          and then, J times each, nothing / only the form's streamed loads /
//          only its stores (`between`)
// The resident share is (miss - case) / (miss - hit) of the medians; a line
// holds every repetition of all three.  `which`: all (default) | kept (the
// kept blocks and between = none only).
struct Sel { unsigned unit_shift, period, window, first; };
template <bool NT>
__global__ __launch_bounds__(256) void kRsel(const v4u* __restrict__ s, v4u* __restrict__ sink, size_t n16, Sel q) {
    const unsigned per = q.window << q.unit_shift, p = blockIdx.x / per, in = blockIdx.x % per;
    const size_t b = ((((size_t)p * q.period + q.first + (in >> q.unit_shift))) << q.unit_shift) + (in & ((1u << q.unit_shift) - 1));
    const size_t i = b * 256 + threadIdx.x;
    v4u r = {0, 0, 0, 0};
    if (i < n16) r = NT ? __builtin_nontemporal_load(s + i) : s[i];
    unsigned x = r.x ^ r.y ^ r.z ^ r.w;
    for (int o = 32; o > 0; o >>= 1) x ^= __shfl_xor(x, o);
    if (x == 0x9e3779b9u && threadIdx.x == 0) sink[blockIdx.x] = r;   // keeps the loads live; blockIdx.x < n / 4096
}
static int keep_lab(size_t n, const char* only, const char* windows, int K, int J, bool kept_only) {
    Lab L = lab_open(n);
    const size_t n16 = n / 16;
    for (const Win& w : win_specs(windows, n)) {
        const unsigned period = w.period_mask + 1;
        const size_t periods = n / ((size_t)period * (4096ull << w.unit_shift));   // whole periods only
        if (!periods || !w.window) { fprintf(stderr, "keep: no whole period or an empty window\n"); return 2; }
        const unsigned grid = (unsigned)(periods * ((size_t)w.window << w.unit_shift));   // <= n / 4096
        const Sel whole = {w.unit_shift, period, period, 0};
        const unsigned whole_grid = (unsigned)(periods * ((size_t)period << w.unit_shift));
        for (const Pol& p : kPols) {
            WinVar v = {"", p.copy, w};
            pol_name(p, w, n, v.name, sizeof v.name);
            if (only ? !strstr(v.name, only) : (&p != &kPols[0])) continue;   // default: the shipped form alone
            for (int target = 0; target < (kept_only ? 1 : 2); ++target) {
                if (target && 2 * w.window > period) continue;   // no room for as many streamed units
                const Sel q = {w.unit_shift, period, w.window, target ? period / 2 : 0};
                for (int between = 0; between < (kept_only ? 1 : 3); ++between) {
                    double t[3][kReps];
                    auto probe = [&](double* out) {
                        float ms;
                        CK(hipEventRecord(L.e0, L.st));
                        hipLaunchKernelGGL(kRsel<true>, dim3(grid), dim3(256), 0, L.st, (const v4u*)L.s[0], (v4u*)L.sink, n16, q);
                        CK(hipEventRecord(L.e1, L.st));
                        CK(hipEventSynchronize(L.e1));
                        CK(hipEventElapsedTime(&ms, L.e0, L.e1));
                        CK(hipGetLastError());
                        *out = ms * 1e3;
                    };
                    auto flush = [&]() {
                        for (int l = 0; l < 2; ++l)
                            for (int pr = 1; pr < L.pairs; ++pr) win_run(v, L.s[pr], L.d[pr], n, L.st);
                        hipLaunchKernelGGL(kRsel<false>, dim3(whole_grid), dim3(256), 0, L.st, (const v4u*)L.s[1], (v4u*)L.sink, n16, whole);
                    };
                    const unsigned g = (unsigned)((n + 4095) / 4096);
                    for (int rep = 0; rep < kReps; ++rep) {
                        for (int l = 0; l < 2; ++l)
                            hipLaunchKernelGGL(kRsel<false>, dim3(grid), dim3(256), 0, L.st, (const v4u*)L.s[0], (v4u*)L.sink, n16, q);
                        probe(&t[0][rep]);
                        flush();
                        probe(&t[1][rep]);
                        flush();
                        for (int l = 0; l < K; ++l) win_run(v, L.s[0], L.d[0], n, L.st);
                        if (between)
                            for (int l = 0; l < J; ++l)
                                hipLaunchKernelGGL(between == 1 ? p.loads : p.stores, dim3(g), dim3(256), 0, L.st,
                                                   (const unsigned char*)L.s[0], between == 1 ? L.sink : (unsigned char*)L.d[0], n, w);
                        probe(&t[2][rep]);
                    }
                    double lo[3], med[3], hi[3];
                    for (int m = 0; m < 3; ++m) win_stats(t[m], kReps, &lo[m], &med[m], &hi[m]);
                    printf("{\"probe\": \"keep\", \"form\": \"%s\", \"bytes\": %zu, \"unit_period_window\": [%u, %u, %u], "
                           "\"target\": \"%s\", \"probed_MiB\": %.1f, \"priming_copies\": %d, \"between\": \"%s\", \"between_runs\": %d",
                           v.name, n, 1u << w.unit_shift, period, w.window, target ? "streamed" : "kept",
                           grid * 4096.0 / (1 << 20), K, between == 0 ? "none" : between == 1 ? "loads" : "stores", between ? J : 0);
                    const char* keys[3] = {"hit_us", "miss_us", "case_us"};
                    for (int m = 0; m < 3; ++m) {
                        printf(", \"%s\": [", keys[m]);
                        for (int rep = 0; rep < kReps; ++rep) printf("%s%.1f", rep ? ", " : "", t[m][rep]);
                        printf("]");
                    }
                    printf(", \"hit_clear_of_miss\": %s, \"resident_share\": %.3f}\n", hi[0] < lo[1] ? "true" : "false",
                           med[1] > med[0] ? (med[1] - med[2]) / (med[1] - med[0]) : 0.0);
                    fflush(stdout);
                }
            }
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    const size_t n = argc > 1 ? strtoull(argv[1], 0, 0) : (1ull << 30);
    if (argc > 2 && !strncmp(argv[2], "win", 3))
        return win_lab(n, argc > 3 ? argv[3] : nullptr, argc > 4 ? argv[4] : nullptr, !strcmp(argv[2], "win2"));
    if (argc > 2 && !strcmp(argv[2], "pol")) return pol_lab(n, argc > 3 ? argv[3] : nullptr, argc > 4 ? argv[4] : nullptr);
    if (argc > 2 && !strcmp(argv[2], "keep"))
        return keep_lab(n, argc > 3 && *argv[3] ? argv[3] : nullptr, argc > 4 ? argv[4] : nullptr, argc > 5 ? atoi(argv[5]) : 3,
                        argc > 6 ? atoi(argv[6]) : 3, argc > 7 && !strcmp(argv[7], "kept"));
    const char* only = argc > 2 ? argv[2] : nullptr;
    // optional placement offsets (argv[3] dst, argv[4] src, bytes): where the
    // two buffers sit relative to each other in the HBM channel interleave
    const size_t doff = argc > 3 ? strtoull(argv[3], 0, 0) : 0, soff = argc > 4 ? strtoull(argv[4], 0, 0) : 0;
    void *s, *d, *s0, *d0;
    unsigned* bad;
    CK(hipMalloc(&s0, n + soff));
    CK(hipMalloc(&d0, n + doff));
    s = (char*)s0 + soff;
    d = (char*)d0 + doff;
    CK(hipMalloc(&bad, 4));
    hipStream_t st;
    CK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    hipLaunchKernelGGL(kfill, dim3(4096), dim3(256), 0, st, (unsigned*)s, n / 4);
    CK(hipStreamSynchronize(st));
    // aux: sc0 = 1, nt = 2, sc1 = 16 (gfx940-family buffer cache policy bits)
    std::vector<Var> vs = {
        {"A_t256_u2_nt_g65536 (product)", 65536, 256, runA<256, 2, true>},
        {"E_t256_u1", 0, 256, runE<256, 1>},
        {"E_t256_u2", 0, 256, runE<256, 2>},
        {"E_t256_u4", 0, 256, runE<256, 4>},
        {"E_t512_u1", 0, 512, runE<512, 1>},
        {"E_t512_u2", 0, 512, runE<512, 2>},
        {"E_t1024_u1", 0, 1024, runE<1024, 1>},
        {"E_t1024_u2", 0, 1024, runE<1024, 2>},
        {"E_t128_u2", 0, 128, runE<128, 2>},
        {"E_t64_u4", 0, 64, runE<64, 4>},
        {"A_t256_u1_nt_g262144", 262144, 256, runA<256, 1, true>},
        {"A_t512_u1_nt_g131072", 131072, 512, runA<512, 1, true>},
        {"M_hipMemcpyAsync_D2D", 0, 0, runM},
        {"R_read_only (rate x0.5 = read GB/s)", 0, 256, runR},
        {"W_write_only (rate x0.5 = write GB/s)", 0, 256, runW},
        {"A_t256_u2_nt_g65536 (product, again)", 65536, 256, runA<256, 2, true>},
        {"E_t256_u1 (again)", 0, 256, runE<256, 1>},
        {"E_t512_u1 (again)", 0, 512, runE<512, 1>},
    };
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    const int L = 20;
    for (const Var& v : vs) {
        if (only && !strstr(v.name, only)) continue;
        CK(hipMemsetAsync(d, 0, n, st));
        v.run(s, d, n, v.grid, v.threads, st);   // warm
        CK(hipGetLastError());
        CK(hipMemsetAsync(bad, 0, 4, st));
        hipLaunchKernelGGL(kcmp, dim3(4096), dim3(256), 0, st, (const unsigned*)s, (const unsigned*)d, n / 4, bad);
        unsigned nb = 0;
        CK(hipMemcpyAsync(&nb, bad, 4, hipMemcpyDeviceToHost, st));
        CK(hipStreamSynchronize(st));
        double best = 0, sum = 0;
        for (int rep = 0; rep < 5; ++rep) {
            CK(hipEventRecord(e0, st));
            for (int l = 0; l < L; ++l) v.run(s, d, n, v.grid, v.threads, st);
            CK(hipEventRecord(e1, st));
            CK(hipEventSynchronize(e1));
            float ms;
            CK(hipEventElapsedTime(&ms, e0, e1));
            const double gbps = 2.0 * n * L / (ms * 1e-3) / 1e9;
            sum += gbps;
            if (gbps > best) best = gbps;
        }
        printf("{\"variant\": \"%s\", \"bytes\": %zu, \"dst_off\": %zu, \"src_off\": %zu, \"hbm_GBps_best\": %.1f, \"hbm_GBps_mean\": %.1f, \"bad_words\": %u}\n",
               v.name, n, doff, soff, best, sum / 5, nb);
        fflush(stdout);
    }
    return 0;
}
