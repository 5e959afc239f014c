// mpx_kernels.hip — CDNA4 (gfx950) device code of libmpx.
//
// Kernels
//   k_copy      local HBM copy, one 16-B unit per lane, one step per block (config 2)
//   k_copy_win  the same with part of src kept in the Infinity Cache (from 512 MiB)
//   k_xfer      the reference's three transfer loops as ONE persistent launch
//               per rank: pushes go straight into the peer's HBM over xGMI,
//               receives are device-side polls of the rank's mailbox
//               (do_mpi_benchmark*, /root/reference/mpi_perf.c:66-145)
//   k_xfer_fan  one rank's blocks to and from several peers in one launch
//               (mpx_xfer_fan): every workgroup owns one chunk of one link
//   k_xfer_fan_ll  the same with MPX_FAN_LL: per link a lock-step exchange of
//               LL granules, one workgroup per link (<CHECK, LAT>: LAT is the
//               form traced per link, mpx_fan_lat_*)
//   k_xfer_hostlink  a GPU rank's side of the ping-pong / unidir loop with a
//               CPU endpoint across PCIe (mpx_xfer_hostlink): the same pushes,
//               and bulk receives pulled from the endpoint's pinned tx
//   k_hostlink_lat  the same loop traced per iteration (mpx_hostlink_lat_*)
//   k_hostlink_gen  the same loop with every push generated from its
//               iteration's key (mpx_xfer_hostlink_seq), untraced
//   k_fill      tx fill (memset 'a'/'b', mpi_perf.c:244-251, or a seeded pattern)
//   k_checksum  order-independent 64-bit payload checksum
//   k_signal / k_wait   one-lane flag store / bounded poll (SDMA engine)
//
// Memory-ordering contract (see DESIGN.md "Hand-off"):
//  * bulk payload: 16-B buffer stores with sc0|sc1 (system-scope write-through),
//    every storing wave `s_waitcnt vmcnt(0)`, workgroup barrier, then ONE lane
//    stores the workgroup's flag with a system-scope relaxed store;
//  * LL payload (<= 8 KiB, or a 1-byte ack): the data IS the flag — 8-byte
//    {tag, 4 payload bytes} granules, each written by one system-scope store;
//  * receivers poll with system-scope relaxed loads (sc0 sc1) and bounded
//    spins (s_memrealtime deadline); after a timeout every workgroup exits.
#include "mpx_internal.h"

namespace mpx {

typedef unsigned int v4u __attribute__((ext_vector_type(4)));

constexpr u64 kGolden = 0x9E3779B97F4A7C15ull;
constexpr int kAuxSys = 17;                 // buffer cache policy: sc0 | sc1
constexpr int kAuxSysNt = 19;               // sc0 | nt | sc1 (MPX_XFER_STREAM)
constexpr int kAuxSysVol = (int)0x80000011u; // sc0 | sc1, volatile (re-issued every poll)
constexpr int kLLUnits = kLLGranules / 2;    // 16-B LL units (two granules each)
constexpr int kLLUnitsPerLane = kLLUnits / kBlock;
constexpr unsigned kRsrcWord3 = 0x00020000; // raw buffer, 32-bit data format

__device__ __forceinline__ u64 mix64(u64 z) {
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
// checksum term of little-endian 64-bit word w at word index k
__device__ __forceinline__ u64 csum_term(u64 w, u64 k) { return mix64(w + (k + 1) * kGolden); }
// MPX_FILL_SPLITMIX word k
__device__ __forceinline__ u64 fill_word(u64 key, u64 k) { return mix64((key ^ k) + kGolden); }

__device__ __forceinline__ u64 ld_sys(const u64* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ void st_sys(u64* p, u64 v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ void drain_stores() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
__device__ __forceinline__ u64 now_ticks() { return __builtin_amdgcn_s_memrealtime(); }

__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const void* base, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, kRsrcWord3);
}

// 64-bit sum over the workgroup; result valid in thread 0.
__device__ __forceinline__ u64 block_sum(u64 v, u64* lds4) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) lds4[wave] = v;
    __syncthreads();
    u64 s = 0;
    if (threadIdx.x == 0) s = lds4[0] + lds4[1] + lds4[2] + lds4[3];
    __syncthreads();
    return s;
}

// ---------------------------------------------------------------------------
// k_copy: dst[0:n) = src[0:n).  n16 = n / 16 vector units; the tail bytes are
// copied by block 0.  Every lane keeps U independent 16-B loads in flight.
//   CONTIG = false: grid-stride over the whole buffer (unit i, i+G, ...)
//   CONTIG = true : block b owns one contiguous chunk, swept 4 KiB per step
//   LDNT / STNT   : nontemporal (streaming) loads / stores
// launch_copy runs one form: U = 1, nontemporal both ways, one step per block.
// ---------------------------------------------------------------------------
template <bool NT>
__device__ __forceinline__ v4u ld16(const v4u* p) {
    if constexpr (NT) return __builtin_nontemporal_load(p);
    else return *p;
}
template <bool NT>
__device__ __forceinline__ void st16(v4u* p, v4u v) {
    if constexpr (NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}

template <int U, bool LDNT, bool STNT, bool CONTIG>
__global__ __launch_bounds__(kBlock) void k_copy(const v4u* __restrict__ src, v4u* __restrict__ dst,
                                                size_t n16, unsigned tail) {
    size_t i, end, stride;
    if constexpr (CONTIG) {
        const size_t per = (n16 + gridDim.x - 1) / gridDim.x;
        const size_t lo = (size_t)blockIdx.x * per;
        end = lo + per < n16 ? lo + per : n16;
        i = lo + threadIdx.x;
        stride = kBlock;
    } else {
        end = n16;
        i = (size_t)blockIdx.x * kBlock + threadIdx.x;
        stride = (size_t)gridDim.x * kBlock;
    }
    for (; i + (U - 1) * stride < end; i += U * stride) {
        v4u r[U];
#pragma unroll
        for (int u = 0; u < U; ++u) r[u] = ld16<LDNT>(src + i + u * stride);
#pragma unroll
        for (int u = 0; u < U; ++u) st16<STNT>(dst + i + u * stride, r[u]);
    }
    for (; i < end; i += stride) st16<STNT>(dst + i, ld16<LDNT>(src + i));
    if (blockIdx.x == 0 && threadIdx.x < tail) {
        const unsigned char* s8 = reinterpret_cast<const unsigned char*>(src + n16);
        unsigned char* d8 = reinterpret_cast<unsigned char*>(dst + n16);
        d8[threadIdx.x] = s8[threadIdx.x];
    }
}

// ---------------------------------------------------------------------------
// k_copy_win: launch_copy's form of k_copy (one 16-B unit per lane, one step
// per block) with the load's cache policy chosen per workgroup (CopyWindow,
// mpx_internal.h).  Workgroup b copies 4 KiB block b; a kept block,
// ((b >> shift) & mask) < units, loads with the default policy so that it
// stays in the Infinity Cache for the next copy of src.  The branch is
// uniform.  The kept load is a buffer load, the streamed one a nontemporal
// pointer load: two loads of one pointer that differ only in the hint are
// merged into one plain load under __restrict__, which drops the hint.
// Every store is a buffer store with sc1 | nt: 7 us of 317 faster per GiB
// than the nontemporal pointer store, with and without reuse, and the window
// stays resident under it (DESIGN.md "The streamed side's policy";
// profiles/copy_window_keep_lab.jsonl).  Write-through, and the kernel's end
// releases every store as before: no fence.  tests/test_copy_window_policy.py
// reads the two constants here and the modifiers in the emitted code.
// ---------------------------------------------------------------------------
constexpr int kCopyWinKeptAux = 0;     // kept loads: the default policy
constexpr int kCopyWinStoreAux = 18;   // every store: sc1 | nt
__global__ __launch_bounds__(kBlock) void k_copy_win(const v4u* __restrict__ src, v4u* __restrict__ dst, size_t n16,
                                                    unsigned tail, unsigned shift, unsigned mask, unsigned units) {
    const size_t first = (size_t)blockIdx.x * kBlock, i = first + threadIdx.x;
    // the descriptors cover this block's whole units only: a lane past n16 loads and stores nothing
    const size_t left = n16 - first;   // >= 0: the grid is ceil(n16 / kBlock), or 1 where n16 is 0
    const unsigned bytes = left < (size_t)kBlock ? (unsigned)left * 16 : kBlock * 16;
    v4u r = {0, 0, 0, 0};
    if (((blockIdx.x >> shift) & mask) < units)
        r = __builtin_amdgcn_raw_buffer_load_b128(rsrc(src + first, bytes), threadIdx.x * 16, 0, kCopyWinKeptAux);
    else if (i < n16)
        r = ld16<true>(src + i);
    __builtin_amdgcn_raw_buffer_store_b128(r, rsrc(dst + first, bytes), threadIdx.x * 16, 0, kCopyWinStoreAux);
    if (blockIdx.x == 0 && threadIdx.x < tail) {   // the tail bytes, as k_copy
        const unsigned char* s8 = reinterpret_cast<const unsigned char*>(src + n16);
        unsigned char* d8 = reinterpret_cast<unsigned char*>(dst + n16);
        d8[threadIdx.x] = s8[threadIdx.x];
    }
}

// ---------------------------------------------------------------------------
// k_copy_steps: all `iters` copies dst[0:n) = src[0:n) of one mpx_copy call in
// ONE launch (the reference's loop, mpi_perf.c:70, run on the device like
// k_xfer runs the pair loop).  Below a few MiB a launch of k_copy costs
// 2.1-2.5 us whatever it moves (profiles/r01_cfg2_copy_sweep.jsonl), so the
// sweep's small sizes measured dispatch, not memory.  Every lane owns the
// same 16-B units every step (grid-stride, U = ceil(n16 / (grid*256)) per
// lane); between steps a grid barrier: one lane per workgroup counts in
// (optionally after draining its stores) and waits for the whole grid, so
// step s+1's loads start only after every store of
// step s was issued — back-to-back copies, not an overlapped pipeline.  The
// grid (<= 4 workgroups per CU, 12 VGPRs) is always co-resident.
// ---------------------------------------------------------------------------
// Each lane issues the loads of up to kCopyStepsBatch of its units before
// the first store, so a step costs about one memory latency per batch, not
// one per unit (the grid is sized to give every lane <= one batch per step
// below 1 MiB).
constexpr int kCopyStepsBatch = 8;

template <int T, bool XCD>
__global__ __launch_bounds__(T) void k_copy_steps(const v4u* __restrict__ src, v4u* __restrict__ dst, size_t n16,
                                                 unsigned tail, int iters, u64* bar, int drain, int one_xcd) {
    // one_xcd: the grid is 8x the working workgroups and only those with
    // blockIdx % 8 == 0 work (the rest exit at once), so that with the
    // round-robin dispatch seen on gfx950 every barrier arrival comes from
    // XCD 0.  A placement heuristic, speed only: dispatch -> XCD placement is
    // undefined (MI355X_MICROARCH.md), and the working set is correct
    // wherever it lands (sized to stay resident; the barrier is bounded)
    if (one_xcd && (blockIdx.x & 7)) return;
    const unsigned wg = one_xcd ? blockIdx.x >> 3 : blockIdx.x;
    const u64 g = one_xcd ? gridDim.x >> 3 : gridDim.x;
    const size_t stride = (size_t)g * T;
    const size_t first = (size_t)wg * T + threadIdx.x;
    // XCD = true: two-level arrival.  Workgroups are dispatched round-robin
    // over the 8 XCDs, so workgroup b counts in on its XCD's counter
    // bar[16 * (1 + b % 8)] (8 counters, 128 B apart, in parallel instead of
    // one hot word); the last arriver of each XCD then counts that XCD in on
    // bar[0].
    const int x = (int)(wg & 7);
    const u64 nx = (g - (u64)x + 7) / 8;            // workgroups on this XCD
    const u64 groups = g < 8 ? g : 8;
    const bool one_unit = n16 <= stride;   // at most one unit per lane: no batch
    __shared__ int s_stop;
    for (int s = 0; s < iters; ++s) {
        if (one_unit) {
            if (first < n16) __builtin_nontemporal_store(__builtin_nontemporal_load(src + first), dst + first);
        } else for (size_t base = first; base < n16; base += kCopyStepsBatch * stride) {
            v4u r[kCopyStepsBatch];
#pragma unroll
            for (int u = 0; u < kCopyStepsBatch; ++u)
                if (base + u * stride < n16) r[u] = __builtin_nontemporal_load(src + base + u * stride);
#pragma unroll
            for (int u = 0; u < kCopyStepsBatch; ++u)
                if (base + u * stride < n16) __builtin_nontemporal_store(r[u], dst + base + u * stride);
        }
        if (wg == 0 && threadIdx.x < tail) {
            const unsigned char* s8 = reinterpret_cast<const unsigned char*>(src + n16);
            reinterpret_cast<unsigned char*>(dst + n16)[threadIdx.x] = s8[threadIdx.x];
        }
        if (s + 1 == iters) break;
        if (drain) drain_stores();
        __syncthreads();
        if (g == 1) continue;                       // one workgroup: __syncthreads is the barrier
        if (threadIdx.x == 0) {
            s_stop = 0;
            u64 want;
            if constexpr (XCD) {
                const u64 old = __hip_atomic_fetch_add(bar + 16 * (1 + x), 1ull, __ATOMIC_RELAXED,
                                                       __HIP_MEMORY_SCOPE_AGENT);
                if (old + 1 == nx * (u64)(s + 1))
                    __hip_atomic_fetch_add(bar, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                want = groups * (u64)(s + 1);
            } else {
                __hip_atomic_fetch_add(bar, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                want = g * (u64)(s + 1);
            }
            // bounded: the grid is sized to be resident, but a workgroup that
            // never arrives must not hold the GPU: after 1 s the workgroup
            // stops and flags bar[1], which mpx_copy reports as a timeout
            const u64 t0 = now_ticks();
            u64 spins = 0;
            while (__hip_atomic_load(bar, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < want) {
                if ((++spins & 255) == 0 && now_ticks() - t0 > 100000000ull) {
                    __hip_atomic_store(&bar[1], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    s_stop = 1;
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
            }
        }
        __syncthreads();
        if (s_stop) return;
    }
}

// ---------------------------------------------------------------------------
// k_copy_pipe: the same `iters` back-to-back copies in ONE launch, for the
// sizes where k_copy_steps pays three memory round trips per copy (loads,
// then the stores' completion — __syncthreads drains them —, then the grid
// barrier's atomic and poll; profiles/r03_copy_cliff_*).  Here a copy's step
// costs about one:
//  * four "copy" waves own UPL 16-B units per lane; copy s+1's loads are
//    issued BEFORE copy s's stores (src is read-only while the copies run,
//    and dst is written only by the stores), so they are in flight during
//    copy s's grid barrier; two register sets, unrolled by two, no moves;
//  * a fifth wave runs the grid barrier: its vector-memory counter holds
//    only the barrier's atomic and poll, so waiting for the poll never waits
//    for the copy waves' stores.  Workgroup barriers are plain s_barrier
//    (no fence: nothing drains); the copy waves wait only for their own
//    loads of the next copy (vmcnt counts in issue order, and those loads
//    are older than this copy's stores).
// Copy s+1's stores are issued only after every workgroup has issued copy
// s's stores (the grid barrier orders issue); the kernel's end makes every
// store visible, as a launch per copy does.
// ---------------------------------------------------------------------------
constexpr int kPipeCopyWaves = 4;
constexpr int kPipeThreads = (kPipeCopyWaves + 1) * 64;   // + the barrier wave
constexpr int kAuxNt = 2;                                 // buffer op: nt (streaming)


__device__ __forceinline__ void wg_barrier_nofence() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // LDS (s_stop) before the barrier
    __builtin_amdgcn_s_barrier();
    // LLVM models s_barrier as touching no memory: without a compiler barrier
    // after it too, the s_stop read or the next copy's stores could be
    // scheduled above it
    asm volatile("" ::: "memory");
}

// Branch-free copy-wave code: every unit is a buffer op whose resource ends at
// n16 units (out-of-range loads return 0, out-of-range stores are dropped),
// so the compiler can count each wait exactly (a guarded unit made it wait
// for every outstanding load, the next copy's included).  The < 16 tail bytes
// go the same way through a resource that is empty except in workgroup 0's
// first wave.
template <int UPL>
// (no __restrict__ on src: with it the optimiser may assume src's bytes never
// change during the kernel and keep the first copy's values for every copy)
__global__ __launch_bounds__(kPipeThreads) void k_copy_pipe(const v4u* src, v4u* dst,
                                                          size_t n16, unsigned tail, int iters, u64* bar,
                                                          int hier) {
    __shared__ int s_stop;
    if (threadIdx.x >= kPipeCopyWaves * 64) {
        // the barrier wave: one grid barrier per copy boundary.  hier = 0:
        // one counter (bar[0]) that every workgroup counts in on and polls.
        // hier = 1 (A/B): workgroup b counts in on its group's counter
        // bar[16 (1 + b % 8)]; the last of a group counts the group in on
        // bar[0]; the last group writes every group's release word
        // bar[16 (9 + g)], which that group's workgroups poll — 8 same-address
        // queues in parallel instead of one.
        const unsigned grid = gridDim.x;
        const unsigned g = blockIdx.x & 7;
        const u64 ng = (grid - g + 7) / 8;                   // workgroups in group g
        const u64 groups = grid < 8 ? grid : 8;
        for (int s = 0; s + 1 < iters; ++s) {
            wg_barrier_nofence();                      // every copy wave issued copy s's stores
            if (threadIdx.x == kPipeCopyWaves * 64) {
                s_stop = 0;
                u64 want;
                const u64* poll;
                if (hier) {
                    const u64 old = __hip_atomic_fetch_add(bar + 16 * (1 + g), 1ull, __ATOMIC_RELAXED,
                                                           __HIP_MEMORY_SCOPE_AGENT);
                    if (old + 1 == ng * (u64)(s + 1)) {
                        const u64 t = __hip_atomic_fetch_add(bar, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (t + 1 == groups * (u64)(s + 1))
                            for (u64 k = 0; k < groups; ++k)
                                __hip_atomic_store(bar + 16 * (9 + k), (u64)(s + 1), __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_AGENT);
                    }
                    want = (u64)(s + 1);
                    poll = bar + 16 * (9 + g);
                } else {
                    __hip_atomic_fetch_add(bar, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    want = (u64)grid * (u64)(s + 1);
                    poll = bar;
                }
                const u64 t0 = now_ticks();
                u64 spins = 0;
                while (__hip_atomic_load(poll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < want) {
                    if ((++spins & 255) == 0 && now_ticks() - t0 > 100000000ull) {
                        // 1 s: a workgroup never arrived (bar[1] -> mpx_copy's fallback)
                        __hip_atomic_store(&bar[1], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        s_stop = 1;
                        break;
                    }
                    __builtin_amdgcn_s_sleep(1);
                }
            }
            wg_barrier_nofence();
            if (s_stop) return;
        }
        return;
    }
    const unsigned stride16 = gridDim.x * (kPipeCopyWaves * 64) * 16u;     // bytes between a lane's units
    const unsigned first16 = (blockIdx.x * (kPipeCopyWaves * 64) + threadIdx.x) * 16u;
    const unsigned body = (unsigned)(n16 * 16);
    const __amdgpu_buffer_rsrc_t rs = rsrc(src, body), rd = rsrc(dst, body);
    // wave-uniform, made scalar so the tail resources live in SGPRs
    const unsigned tb = __builtin_amdgcn_readfirstlane((blockIdx.x == 0 && threadIdx.x < 64) ? tail : 0u);
    const __amdgpu_buffer_rsrc_t ts = rsrc(reinterpret_cast<const unsigned char*>(src) + body, tb);
    const __amdgpu_buffer_rsrc_t td = rsrc(reinterpret_cast<unsigned char*>(dst) + body, tb);
    v4u a[UPL], b[UPL];
    unsigned char ta, tb8;
    auto load = [&](v4u (&r)[UPL], unsigned char& t) {
        // a compiler barrier: the buffer-load builtin is a plain memory read to
        // the optimiser, which would otherwise reuse the previous copy's values
        asm volatile("" ::: "memory");
#pragma unroll
        for (int u = 0; u < UPL; ++u)
            r[u] = __builtin_amdgcn_raw_buffer_load_b128(rs, first16 + u * stride16, 0, kAuxNt);
        t = __builtin_amdgcn_raw_buffer_load_b8(ts, threadIdx.x, 0, 0);
    };
    auto store = [&](v4u (&r)[UPL], unsigned char t) {
#pragma unroll
        for (int u = 0; u < UPL; ++u)
            __builtin_amdgcn_raw_buffer_store_b128(r[u], rd, first16 + u * stride16, 0, kAuxNt);
        __builtin_amdgcn_raw_buffer_store_b8(t, td, threadIdx.x, 0, 0);
    };
    // both workgroup barriers of a grid barrier; false: the barrier gave up
    auto grid_barrier = [&]() -> bool {
        wg_barrier_nofence();
        wg_barrier_nofence();
        return !s_stop;
    };
    // copy s+1's loads are issued before copy s's stores (src is read-only
    // while the copies run), so they fly during copy s's grid barrier
    load(a, ta);
    for (int s = 0;;) {
        if (s + 1 == iters) { store(a, ta); break; }
        load(b, tb8);
        store(a, ta);
        if (!grid_barrier()) break;
        if (++s + 1 == iters) { store(b, tb8); break; }
        load(a, ta);
        store(b, tb8);
        if (!grid_barrier()) break;
        ++s;
    }
}

// ---------------------------------------------------------------------------
// k_fill
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_fill(unsigned char* p, size_t n, int pattern, u64 arg) {
    const size_t nw = n / 8;
    const size_t stride = (size_t)gridDim.x * kBlock;
    u64* p64 = reinterpret_cast<u64*>(p);
    const u64 bytew = (arg & 0xff) * 0x0101010101010101ull;
    for (size_t k = (size_t)blockIdx.x * kBlock + threadIdx.x; k < nw; k += stride)
        p64[k] = pattern == MPX_FILL_BYTE ? bytew : fill_word(arg, k);
    const unsigned tail = (unsigned)(n & 7);
    if (blockIdx.x == 0 && threadIdx.x < tail) {
        const u64 w = pattern == MPX_FILL_BYTE ? bytew : fill_word(arg, nw);
        p[nw * 8 + threadIdx.x] = (unsigned char)(w >> (8 * threadIdx.x));
    }
}

// ---------------------------------------------------------------------------
// k_checksum: *out += sum_k csum_term(word_k, k) over the zero-padded 64-bit
// words of p[0:n).  Integer adds commute, so the result is bit-exact whatever
// the order; the host finishes it with ^ mix64(n).
// ---------------------------------------------------------------------------
__device__ __forceinline__ u64 tail_word(const unsigned char* p, size_t off, size_t n) {
    u64 w = 0;
    for (size_t b = 0; off + b < n && b < 8; ++b) w |= (u64)p[off + b] << (8 * b);
    return w;
}

__global__ __launch_bounds__(kBlock) void k_checksum(const unsigned char* p, size_t n, u64* out) {
    __shared__ u64 lds4[4];
    const size_t n16 = n / 16;
    const size_t stride = (size_t)gridDim.x * kBlock;
    const v4u* p16 = reinterpret_cast<const v4u*>(p);
    u64 acc = 0;
    for (size_t v = (size_t)blockIdx.x * kBlock + threadIdx.x; v < n16; v += stride) {
        const v4u x = p16[v];
        acc += csum_term(((u64)x.y << 32) | x.x, 2 * v);
        acc += csum_term(((u64)x.w << 32) | x.z, 2 * v + 1);
    }
    if (blockIdx.x == 0 && threadIdx.x < 2) {
        const size_t off = n16 * 16 + 8 * threadIdx.x;
        if (off < n) acc += csum_term(tail_word(p, off, n), off / 8);
    }
    const u64 s = block_sum(acc, lds4);
    if (threadIdx.x == 0 && s) atomicAdd(out, s);
}

// ---------------------------------------------------------------------------
// SDMA-engine helpers: one lane stores / polls a mailbox flag.  The value is
// v, plus *base when base is set: a graph-captured chunk of the loop
// (run_sdma) carries sequence numbers relative to a device-side base that
// k_seqbase sets before the first replay and advances at the end of each.
// ---------------------------------------------------------------------------
__device__ __forceinline__ u64 rel(const u64* base, u64 v) { return base ? ld_sys(base) + v : v; }

__global__ void k_signal(u64* flag, const u64* base, u64 v) {
    if (threadIdx.x == 0) st_sys(flag, rel(base, v));
}

// A wait of a call whose earlier wait already gave up returns at once: the
// stream then drains in microseconds instead of one deadline per remaining
// wait (a peer that stopped — e.g. its process exited on an error — would
// otherwise hold this stream, and the exit of this process, for deadline x
// the hundreds of waits a checked loop enqueues).
__global__ void k_wait(const u64* flag, const u64* base, u64 v, Status* st, u64 timeout_ticks) {
    if (threadIdx.x != 0) return;
    if (__hip_atomic_load(&st->err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) return;
    const u64 want = rel(base, v);
    const u64 t0 = now_ticks();
    u64 spins = 0, seen;
    while ((seen = ld_sys(flag)) < want) {
        if ((++spins & 255) == 0 && now_ticks() - t0 > timeout_ticks) {
            st->seen = seen;   // diagnostics, read by the host after the stream drains
            st->want = want;
            __hip_atomic_store(&st->err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            return;
        }
        __builtin_amdgcn_s_sleep(1);
    }
}

// base[0..1] = {tx, rx} (add = 0), or base[0..1] += {tx, rx} (add = 1)
__global__ void k_seqbase(u64* base, u64 tx, u64 rx, int add) {
    if (threadIdx.x != 0) return;
    st_sys(base, add ? ld_sys(base) + tx : tx);
    st_sys(base + 1, add ? ld_sys(base + 1) + rx : rx);
}

// ---------------------------------------------------------------------------
// k_xfer: the transfer loop.  One launch runs all `iters` iterations of one
// rank's side; the peer runs its own launch on its own GPU at the same time.
// ---------------------------------------------------------------------------
// phase stamps of workgroup 0 (Loop::ts)
enum { kTsEntry = 0, kTsPosted = 1, kTsFirst = 2, kTsLoop = 3 };

// ANYWG: every workgroup owns an LL message of its own (k_xfer_fan_ll: one
// link per workgroup); false: a pair's LL message is workgroup 0's.
// SEQ: where a push's bytes come from.  false: tx, the same bytes in every
// iteration (staged in LDS, or preloaded for LL); true: generated in
// registers from the iteration's key (mpx_xfer_seq: gen_ll, gen_units), with
// the same stores, chunks, flags and publish schedule.
template <int MODE, bool ANYWG = false, bool SEQ = false>
struct Loop {
    const XferArgs& a;
    int* s_abort;      // LDS: this workgroup gave up
    u64* lds4;         // LDS scratch for block_sum
    v4u* s_tx;         // LDS: this workgroup's staged chunk of tx (a.stage)
    // LL payload of this side's sends, held in VGPRs for the whole launch:
    // pre[j] = tx bytes [8u, 8u+8) of unit u = threadIdx.x + j*kBlock.  tx is
    // read-only while the loop runs (the reference re-sends the same buffer
    // every iteration, mpi_perf.c:72,80,135), so a send is stores only — no
    // tx load on the latency path.
    // 16-B LL units per lane: a pair's message fills the row, an LL fan's half of it
    static constexpr int kUnits = ANYWG ? kLLUnitsPerLane / 2 : kLLUnitsPerLane;
    u64 pre[kUnits];
    u64* s_seen = nullptr;   // LDS, pull mode: the peer's ready word as last read
    // a.stage: s_tx holds this workgroup's chunk once the first push (which
    // reads tx from memory and fills s_tx on the way) is done
    mutable bool staged = false;
    mutable u64 ts[4] = {0, 0, 0, 0};   // workgroup 0's phase stamps (stamp)
    mutable u64 rdone = 0, rdig = 0;    // workgroup 0, thread 0: the call's receive
                                        // count and digest (finish_last writes them)
    // ANYWG: the workgroup's index within its link or direction, the w of its
    // chunk, flag and credit words (k_hostlink_duplex: blockIdx.x less the
    // pushing half of the grid); a pair's is blockIdx.x itself
    int wg_ = 0;
    __device__ unsigned wg() const { return ANYWG ? (unsigned)wg_ : blockIdx.x; }

    __device__ void preload_ll(long long n) {
#pragma unroll
        for (int j = 0; j < kUnits; ++j) {
            const long long off = 8ll * ((int)threadIdx.x + j * kBlock);
            u64 w = 0;
            if (off + 8 <= n) {
                w = *reinterpret_cast<const u64*>(a.tx + off);
            } else {
                for (long long b = 0; off + b < n; ++b) w |= (u64)a.tx[off + b] << (8 * b);
            }
            pre[j] = w;
        }
    }

    // SEQ: the LL payload of iteration key's send, regenerated by the lanes
    // that own units; bytes past n are zero, as preload_ll leaves them
    __device__ void gen_ll(long long n, u64 key) {
#pragma unroll
        for (int j = 0; j < kUnits; ++j) {
            const int u = (int)threadIdx.x + j * kBlock;
            const long long off = 8ll * u;
            u64 w = 0;
            if (off < n) {
                w = fill_word(key, (u64)u);
                if (off + 8 > n) w &= (1ull << (8 * (int)(n - off))) - 1;
            }
            pre[j] = w;
        }
    }

    __device__ bool aborted() const { return *s_abort != 0; }
    __device__ bool ll_owner() const { return ANYWG || blockIdx.x == 0; }

    // Record a timeout: LDS flag for this workgroup, device word for the
    // others (scratch[1]), host-mapped status for the host.
    __device__ void give_up(int iter) const {
        *s_abort = 1;
        __hip_atomic_store(&a.gbar[1], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&a.status->where, (unsigned)iter + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&a.status->err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    // every 64 spins: deadline or another workgroup's abort
    __device__ bool should_stop(u64 spins, u64 t0) const {
        if ((spins & 63) != 0) return false;
        if (*s_abort) return true;
        if (__hip_atomic_load(&a.gbar[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return true;
        return now_ticks() - t0 > a.timeout_ticks;
    }

    __device__ bool is_ll(long long n) const { return MODE != MPX_MODE_NONBLOCKING && n <= a.ll_max; }

    // ---- send: push n bytes of tx[0:n) into the peer's rx -------------------
    // LL: one workgroup; every 16-B store carries two granules {payload:32,
    // tag:32} (each 8-B half lands untorn), so 8 payload bytes per store.
    // goff: the granule of the peer's landing row the message starts at (the
    // LL fan's half, kFanLLHalf * (seq & 1); a pair's message starts at 0).
    __device__ void push_ll(long long n, u64 seq, unsigned goff = 0) const {
        if (!ll_owner()) return;
        const int ng = n > 0 ? (int)((n + 3) >> 2) : 1;   // a 0-byte message is one empty granule
        const int nu = (ng + 1) >> 1;                      // 16-B units
        const unsigned tag = ll_tag(seq);
        const __amdgpu_buffer_rsrc_t dst = rsrc(&a.peer_mb->ll[a.my_slot][goff], (unsigned)(nu * 16));
#pragma unroll
        for (int j = 0; j < kUnits; ++j) {
            const int u = (int)threadIdx.x + j * kBlock;
            if (u < nu) {
                const v4u v = {(unsigned)pre[j], tag, (unsigned)(pre[j] >> 32), tag};
                __builtin_amdgcn_raw_buffer_store_b128(v, dst, (unsigned)u * 16, 0, kAuxSys);
            }
        }
    }

    // this workgroup's chunk [lo, hi) of a bulk push of n bytes
    __device__ void chunk_of(long long n, long long* lo, long long* hi) const {
        const long long chunk = (((n + a.nwg - 1) / a.nwg) + 15) & ~15ll;
        *lo = (long long)wg() * chunk;
        *hi = *lo + chunk < n ? *lo + chunk : n;
    }

    // LDS staging (a.stage): each pushing workgroup keeps its chunk's 16-B
    // units of tx in LDS for the whole launch; every push after the first
    // reads LDS (ds_read_b128) instead of HBM/L2, so the per-iteration
    // critical path is LDS -> remote store.  The first push reads tx from
    // memory and fills LDS on the way (STAGE below): no separate staging pass
    // stands between the start of the call and its first byte on the link.
    // tx is read-only while the loop runs.  Lane t handles units t, t+kBlock,
    // ... in every pass, so it reads back only LDS words it wrote itself.
    template <int AUX, bool STAGE>
    __device__ __forceinline__ void push_units(const v4u* src, __amdgpu_buffer_rsrc_t dst, int nv) const {
        int v = threadIdx.x;
        for (; v + 3 * kBlock < nv; v += 4 * kBlock) {
            const v4u r0 = src[v], r1 = src[v + kBlock], r2 = src[v + 2 * kBlock], r3 = src[v + 3 * kBlock];
            __builtin_amdgcn_raw_buffer_store_b128(r0, dst, v * 16, 0, AUX);
            __builtin_amdgcn_raw_buffer_store_b128(r1, dst, (v + kBlock) * 16, 0, AUX);
            __builtin_amdgcn_raw_buffer_store_b128(r2, dst, (v + 2 * kBlock) * 16, 0, AUX);
            __builtin_amdgcn_raw_buffer_store_b128(r3, dst, (v + 3 * kBlock) * 16, 0, AUX);
            if (STAGE) {
                s_tx[v] = r0;
                s_tx[v + kBlock] = r1;
                s_tx[v + 2 * kBlock] = r2;
                s_tx[v + 3 * kBlock] = r3;
            }
        }
        for (; v < nv; v += kBlock) {
            const v4u r = src[v];
            __builtin_amdgcn_raw_buffer_store_b128(r, dst, v * 16, 0, AUX);
            if (STAGE) s_tx[v] = r;
        }
    }
    template <bool STAGE>
    __device__ __forceinline__ void push_units_aux(const v4u* src, __amdgpu_buffer_rsrc_t dst, int nv) const {
        if (a.stream) push_units<kAuxSysNt, STAGE>(src, dst, nv);
        else push_units<kAuxSys, STAGE>(src, dst, nv);
    }

    // SEQ: the chunk's 16-B units generated instead of read: unit v of a chunk
    // whose first 64-bit word is k0 (lo / 8) holds words k0 + 2v and k0 + 2v + 1
    // of the iteration's pattern.  The same 4-deep batches of stores.
    __device__ __forceinline__ v4u gen16(u64 key, u64 k) const {
        const u64 w0 = fill_word(key, k), w1 = fill_word(key, k + 1);
        return v4u{(unsigned)w0, (unsigned)(w0 >> 32), (unsigned)w1, (unsigned)(w1 >> 32)};
    }
    template <int AUX>
    __device__ __forceinline__ void gen_units(__amdgpu_buffer_rsrc_t dst, int nv, u64 key, u64 k0) const {
        int v = threadIdx.x;
        for (; v + 3 * kBlock < nv; v += 4 * kBlock) {
            const v4u r0 = gen16(key, k0 + 2 * (u64)v), r1 = gen16(key, k0 + 2 * (u64)(v + kBlock)),
                      r2 = gen16(key, k0 + 2 * (u64)(v + 2 * kBlock)), r3 = gen16(key, k0 + 2 * (u64)(v + 3 * kBlock));
            __builtin_amdgcn_raw_buffer_store_b128(r0, dst, v * 16, 0, AUX);
            __builtin_amdgcn_raw_buffer_store_b128(r1, dst, (v + kBlock) * 16, 0, AUX);
            __builtin_amdgcn_raw_buffer_store_b128(r2, dst, (v + 2 * kBlock) * 16, 0, AUX);
            __builtin_amdgcn_raw_buffer_store_b128(r3, dst, (v + 3 * kBlock) * 16, 0, AUX);
        }
        for (; v < nv; v += kBlock)
            __builtin_amdgcn_raw_buffer_store_b128(gen16(key, k0 + 2 * (u64)v), dst, v * 16, 0, AUX);
    }

    // publish = false: the stores are issued but not drained and no flag is
    // stored (non-blocking mode publishes every a.nb_publish pushes, see k_xfer).
    // dst_base: the peer's receive slot (default: its rx).  skip (test knob
    // MPX_TEST_SKIP_PUSH): no payload stores, the flag is still published.
    // key (SEQ): the iteration's pattern key; skip then skips generation too.
    __device__ void push_bulk(long long n, u64 seq, bool publish = true, unsigned char* dst_base = nullptr,
                              bool skip = false, u64 key = 0) const {
        const int w = wg();
        if (w >= a.nwg) return;
        long long lo, hi;
        chunk_of(n, &lo, &hi);
        if constexpr (SEQ) {
            if (lo < hi && !skip) {
                const unsigned bytes = (unsigned)(hi - lo);
                const __amdgpu_buffer_rsrc_t dst = rsrc((dst_base ? dst_base : a.peer_rx) + lo, bytes);
                const int nv = (int)(bytes >> 4);
                const u64 k0 = (u64)lo >> 3;               // lo is a multiple of 16
                if (a.stream) gen_units<kAuxSysNt>(dst, nv, key, k0);
                else gen_units<kAuxSys>(dst, nv, key, k0);
                const unsigned tail = bytes & 15;          // only the last workgroup: the one or two words they fall in
                if (threadIdx.x < tail) {
                    const unsigned o = (unsigned)nv * 16 + threadIdx.x;
                    const u64 wd = fill_word(key, k0 + (o >> 3));
                    __builtin_amdgcn_raw_buffer_store_b8((unsigned char)(wd >> (8 * (o & 7))), dst, o, 0, kAuxSys);
                }
            }
        } else if (lo < hi) {
            const unsigned bytes = (unsigned)(hi - lo);
            const __amdgpu_buffer_rsrc_t dst = rsrc((dst_base ? dst_base : a.peer_rx) + lo, bytes);
            const int nv = (int)(bytes >> 4);
            const v4u* txv = reinterpret_cast<const v4u*>(a.tx + lo);
            if (a.stage && !staged) {
                if (!skip) {
                    push_units_aux<true>(txv, dst, nv);
                } else {
                    for (int v = threadIdx.x; v < nv; v += kBlock) s_tx[v] = txv[v];   // stage only
                }
            } else if (!skip) {
                push_units_aux<false>(a.stage ? s_tx : txv, dst, nv);
            }
            const unsigned tail = bytes & 15;
            if (threadIdx.x < tail && !skip) {
                const unsigned o = (unsigned)nv * 16 + threadIdx.x;
                __builtin_amdgcn_raw_buffer_store_b8(a.tx[lo + o], dst, o, 0, kAuxSys);
            }
        }
        staged = true;
        if (!publish) return;
        drain_stores();                 // every storing wave
        __syncthreads();
        if (threadIdx.x == 0) st_sys(&a.peer_mb->flag[a.my_slot][w], seq);
    }

    __device__ void send(long long n, u64 seq, bool skip = false, u64 key = 0) const {
        if (is_ll(n)) { if (!skip) push_ll(n, seq); else push_ll_tags_only(n, seq); }
        else push_bulk(n, seq, true, nullptr, skip, key);
    }

    // test knob: an LL message whose payload was "lost" — the tags arrive (so
    // the receiver completes), the data words carry a fixed wrong pattern
    __device__ void push_ll_tags_only(long long n, u64 seq, unsigned goff = 0) const {
        if (!ll_owner()) return;
        const int ng = n > 0 ? (int)((n + 3) >> 2) : 1;
        const int nu = (ng + 1) >> 1;
        const unsigned tag = ll_tag(seq);
        const __amdgpu_buffer_rsrc_t dst = rsrc(&a.peer_mb->ll[a.my_slot][goff], (unsigned)(nu * 16));
        for (int u = threadIdx.x; u < nu; u += kBlock) {
            const v4u v = {~0u, tag, ~0u, tag};
            __builtin_amdgcn_raw_buffer_store_b128(v, dst, (unsigned)u * 16, 0, kAuxSys);
        }
    }

    // ---- receive: wait until the peer's push `seq` of n bytes has landed ----
    // LL receive: every lane issues the loads of ALL its units (up to 4)
    // back to back, then checks the tags — one memory round trip per poll,
    // not one per unit.
    // One 16-B sc0|sc1 volatile load per unit, both granule tags checked
    // (the sender tags both halves of every unit).  Against the earlier 8-B
    // granule loads it halves the load count: 4 KiB ping-pong 4.32 -> 2.56 us
    // per iteration (profiles/r01_ll_ab.jsonl, r01_ll_preload_ab.jsonl).
    __device__ bool wait_ll(long long n, u64 seq, int iter, unsigned goff = 0) const {
        const int ng = n > 0 ? (int)((n + 3) >> 2) : 1;
        const int nu = (ng + 1) >> 1;
        const int mine = nu > (int)threadIdx.x ? (nu - (int)threadIdx.x + kBlock - 1) / kBlock : 0;
        const unsigned tag = ll_tag(seq);
        const __amdgpu_buffer_rsrc_t src = rsrc(&a.my_mb->ll[a.peer_slot][goff], (unsigned)(nu * 16));
        v4u x[kUnits];
        if (mine > 0) {
            const u64 t0 = now_ticks();
            u64 spins = 0;
            for (;;) {
#pragma unroll
                for (int j = 0; j < kUnits; ++j)
                    if (j < mine)
                        x[j] = __builtin_amdgcn_raw_buffer_load_b128(src, ((unsigned)threadIdx.x + j * kBlock) * 16, 0,
                                                                     kAuxSysVol);
                bool ok = true;
#pragma unroll
                for (int j = 0; j < kUnits; ++j)
                    if (j < mine) ok &= (x[j].y == tag) & (x[j].w == tag);
                if (ok) break;
                if (should_stop(++spins, t0)) { give_up(iter); break; }
                __builtin_amdgcn_s_sleep(0);
            }
            if (ll_owner() && !*s_abort) {
                // write-through (sc0 sc1) like every other store into rx, so
                // the bytes are in memory once the call's completion word is
                const __amdgpu_buffer_rsrc_t rr = rsrc(a.rx, (unsigned)n);
#pragma unroll
                for (int j = 0; j < kUnits; ++j) {
                    if (j >= mine) break;
                    const long long off = 8ll * ((int)threadIdx.x + j * kBlock);
                    const u64 d = ((u64)x[j].z << 32) | x[j].x;
                    if (off + 8 <= n) {
                        const unsigned lo = (unsigned)d, hi = (unsigned)(d >> 32);
                        __builtin_amdgcn_raw_buffer_store_b32(lo, rr, (unsigned)off, 0, kAuxSys);
                        __builtin_amdgcn_raw_buffer_store_b32(hi, rr, (unsigned)off + 4, 0, kAuxSys);
                    } else {
                        for (long long b = 0; off + b < n; ++b)
                            __builtin_amdgcn_raw_buffer_store_b8((unsigned char)(d >> (8 * b)), rr, (unsigned)(off + b),
                                                                 0, kAuxSys);
                    }
                }
            }
        }
        __syncthreads();
        return !aborted();
    }

    __device__ bool wait_bulk(u64 seq, int iter) const {
        if (threadIdx.x < 64) {
            const u64* f = &a.my_mb->flag[a.peer_slot][0];
            const u64 t0 = now_ticks();
            u64 spins = 0;
            for (;;) {
                bool ok = true;
                for (int j = threadIdx.x; j < a.nwg; j += 64) ok &= ld_sys(f + j) >= seq;
                if (__all(ok)) break;
                if (should_stop(++spins, t0)) {
                    if (threadIdx.x == 0) give_up(iter);
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
            }
        }
        __syncthreads();
        return !aborted();
    }

    __device__ bool recv(long long n, u64 seq, int iter) const {
        return is_ll(n) ? wait_ll(n, seq, iter) : wait_bulk(seq, iter);
    }

    // ---- matched-receive order (Mailbox.posted) -----------------------------
    // This call's receives are posted: the peer may now push its call a.call
    // into this rank's rx / ring / LL zone.  The kernel is the first command
    // of the call on this rank's stream, so every workgroup of the previous
    // call has finished (checks, poison stores and all) and the host has
    // finished whatever it did with rx between the calls.
    __device__ void post_receives() const {
        if (blockIdx.x == 0 && threadIdx.x == 0) st_sys(&a.peer_mb->posted[a.my_slot], a.call);
    }
    __device__ bool peer_posted() const { return ld_sys(&a.my_mb->posted[a.peer_slot]) >= a.call; }
    // Before this side's first push of the call: wait for the peer's post.
    // Once per call, not per iteration.
    __device__ bool wait_posted() const {
        if (threadIdx.x == 0) {
            const u64 t0 = now_ticks();
            u64 spins = 0;
            while (!peer_posted()) {
                if (should_stop(++spins, t0)) { give_up(0); break; }
                __builtin_amdgcn_s_sleep(1);
            }
        }
        stamp(kTsPosted);
        __syncthreads();
        return !aborted();
    }

    // ---- check mode: checksum the received payload, then poison it ----------
    // The poison guarantees the NEXT iteration's checksum only passes if the
    // next payload really overwrote every byte.
    // The last iteration is not poisoned: rx ends holding the last payload,
    // as the reference's rx does.
    __device__ void check(long long n, int iter) const {
        const u64 poison = 0x5a5a5a5a5a5a5a5aull ^ (u64)iter;
        const bool last = iter + 1 == a.iters;
        u64 acc = 0;
        if (is_ll(n)) {
            // unpacked by workgroup 0 with write-through stores: read back
            // the same way (sc0 sc1 loads: no L1 line of an earlier
            // iteration's read can serve them)
            if (ll_owner()) {
                const __amdgpu_buffer_rsrc_t rr = rsrc(a.rx, (unsigned)n);
                for (long long k = threadIdx.x; 8 * k < n; k += kBlock) {
                    const unsigned o = (unsigned)(8 * k);
                    u64 w = 0;
                    if (8 * k + 8 <= n) {
                        w = (u64)__builtin_amdgcn_raw_buffer_load_b32(rr, o, 0, kAuxSys) |
                            ((u64)__builtin_amdgcn_raw_buffer_load_b32(rr, o + 4, 0, kAuxSys) << 32);
                    } else {
                        for (long long b = 0; 8 * k + b < n; ++b)
                            w |= (u64)__builtin_amdgcn_raw_buffer_load_b8(rr, o + (unsigned)b, 0, kAuxSys) << (8 * b);
                    }
                    acc += csum_term(w, k);
                }
                __syncthreads();
                if (!last) {
                    for (long long o = threadIdx.x; o < n; o += kBlock)
                        __builtin_amdgcn_raw_buffer_store_b8((unsigned char)poison, rr, (unsigned)o, 0, kAuxSys);
                    drain_stores();   // the poison lands before the next payload's unpack
                }
            }
        } else if ((int)wg() < a.nwg) {
            acc = sum_chunk(a.rx, n, poison, last);
        }
        const u64 s = block_sum(acc, lds4);
        if (threadIdx.x == 0 && s) atomicAdd(&a.csum[iter], s);
    }

    // This workgroup's chunk of a bulk payload of n bytes at `base` that the
    // peer stored: system-scope acquire, sc0|sc1 loads, the lane's partial
    // checksum returned; then poison stores (write-through) unless `keep`,
    // drained before returning.
    __device__ u64 sum_chunk(unsigned char* base, long long n, u64 poison, bool keep) const {
        u64 acc = 0;
        if (threadIdx.x == 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
        drain_stores();
        __syncthreads();
        long long lo, hi;
        chunk_of(n, &lo, &hi);
        if (lo < hi) {
            const unsigned bytes = (unsigned)(hi - lo);
            const __amdgpu_buffer_rsrc_t r = rsrc(base + lo, bytes);
            const int nv = (int)(bytes >> 4);
            const v4u pv = {(unsigned)poison, (unsigned)(poison >> 32), (unsigned)poison, (unsigned)(poison >> 32)};
            for (int v = threadIdx.x; v < nv; v += kBlock) {
                const v4u x = __builtin_amdgcn_raw_buffer_load_b128(r, v * 16, 0, kAuxSys);
                const u64 k = (u64)(lo / 8) + 2 * (u64)v;
                acc += csum_term(((u64)x.y << 32) | x.x, k);
                acc += csum_term(((u64)x.w << 32) | x.z, k + 1);
                if (!keep) __builtin_amdgcn_raw_buffer_store_b128(pv, r, v * 16, 0, kAuxSys);
            }
            const unsigned tail = bytes & 15;   // only the last workgroup
            if (threadIdx.x < 2 && 8 * threadIdx.x < tail) {
                const long long off = lo + (long long)nv * 16 + 8 * threadIdx.x;
                u64 w = 0;
                for (long long b = 0; b < 8 && off + b < n; ++b) {
                    const unsigned char c = __builtin_amdgcn_raw_buffer_load_b8(r, (unsigned)(off - lo + b), 0, kAuxSys);
                    w |= (u64)c << (8 * b);
                }
                acc += csum_term(w, (u64)off / 8);
            }
            __syncthreads();
            if (!keep && threadIdx.x < tail)
                __builtin_amdgcn_raw_buffer_store_b8((unsigned char)poison, r, (unsigned)nv * 16 + threadIdx.x, 0, kAuxSys);
        }
        drain_stores();
        return acc;
    }

    // ---- receive accounting ------------------------------------------------
    // Ping-pong / unidir: every receive is counted when it completes (a
    // blocking Recv).  At the end the last workgroup to finish (all chunk
    // checksums are in by then) adds up the finished checksums of the `done`
    // receives (check mode) and stores the count and digest.
    __device__ void account(u64 done, long long n_recv) const {
        u64 part = 0;
        if (a.check) {
            const u64 fmix = mix64((u64)n_recv);
            for (u64 j = threadIdx.x; j < done; j += kBlock)
                part += __hip_atomic_load(&a.csum[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ^ fmix;
        }
        const u64 s = a.check ? block_sum(part, lds4) : 0;
        if (threadIdx.x == 0) {
            rdone = done;
            rdig = s;
        }
    }

    // ---- armed calls (mpx_xfer_arm) ----------------------------------------
    // The kernel was launched before the host's barrier; the loop starts when
    // the host stores this call's token into Status.go (mpx_xfer_ex after the
    // barrier) — MPI's persistent-request split (MPI_Send_init ... MPI_Start).
    // Workgroup 0 polls the host word and hands its verdict to the others in
    // scratch word kScrGo.  False: cancelled (mpx_xfer_disarm) or no start
    // within go_timeout_ticks (then Status.err = 2): no transfer at all.
    // Every other workgroup counts itself in (kScrReady) when it starts to
    // wait; once all have, workgroup 0 stores the token into Status.ready —
    // the whole grid is resident and waiting — which mpx_xfer_arm waits for,
    // so a start right after the host's barrier does not also pay the rest of
    // the launch.
    __device__ bool wait_go() const {
        if (!a.go_token) return true;
        __shared__ int s_go;
        if (threadIdx.x == 0) {
            const u64 t0 = now_ticks();
            u64 spins = 0, w = 0;
            if (blockIdx.x == 0) {
                bool told = false;
                for (;;) {
                    if (!told && __hip_atomic_load(&a.gbar[kScrReady], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ==
                                     (u64)gridDim.x - 1) {
                        st_sys(&a.status->ready, a.go_token);
                        told = true;
                    }
                    const u64 v = ld_sys(&a.status->go);
                    if (v == a.go_token) { w = 1; break; }
                    if (v == (a.go_token | kGoCancel)) { w = 2; break; }
                    if ((++spins & 63) == 0 && now_ticks() - t0 > a.go_timeout_ticks) {
                        __hip_atomic_store(&a.status->err, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                        w = 2;
                        break;
                    }
                    __builtin_amdgcn_s_sleep(2);
                }
                __hip_atomic_store(&a.gbar[kScrGo], w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else {
                __hip_atomic_fetch_add(&a.gbar[kScrReady], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                // (workgroup 0 answers within its own deadline; one second
                // more bounds this wait should it never run)
                while ((w = __hip_atomic_load(&a.gbar[kScrGo], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == 0) {
                    if ((++spins & 63) == 0 && now_ticks() - t0 > a.go_timeout_ticks + 100000000ull) { w = 2; break; }
                    __builtin_amdgcn_s_sleep(2);
                }
            }
            s_go = (int)w;
        }
        __syncthreads();
        return s_go == 1;
    }

    // ---- call phases and the end of the call --------------------------------
    // Workgroup 0 stamps the call's start (Status.t_entry) as its first action
    // and, on a side that pushes first, the moment the peer's receives were
    // seen posted (t_posted): the host splits a call's wall time into launch,
    // wait for the peer, transfer and completion with them (mpx_last_phases).
    // The stamps stay in workgroup 0's registers (ts) until it ends the call
    // (finish_last): a store to host memory here would make the loop's next
    // drain wait for its PCIe round trip.
    __device__ void stamp(int k) const {
        if (blockIdx.x == 0 && threadIdx.x == 0) ts[k] = now_ticks();
    }
    // Every workgroup calls it last.  Workgroup 0 ends the call: the others
    // count themselves out (release) and exit; workgroup 0 waits until all
    // have (acquire) — they are done with the scratch words, the status
    // fields and their checksums by then — and returns true.  The others end
    // early where they can (the last receive of a side that only waits for
    // it, see k_xfer), so their count is usually in before workgroup 0 looks.
    __device__ bool last_to_finish() const {
        drain_stores();    // every wave: its stores of the call (rx unpacks, poison) are in memory
        __syncthreads();
        if (gridDim.x == 1) return true;   // (no counter round trip for a 1-workgroup grid)
        // What workgroup 0 needs from the others is in memory once their
        // waves have drained (above): their payload, poison and rx stores
        // are write-through (sc0 sc1) and their checksums atomics.  So the
        // count is a relaxed add after the drain — an agent-scope release
        // would add an L2 write-back (buffer_wbl2) with nothing to write —
        // and workgroup 0 polls it with relaxed loads and invalidates (one
        // acquire) once, not on every poll.
        if (blockIdx.x != 0) {
            if (threadIdx.x == 0)
                __hip_atomic_fetch_add(&a.gbar[kScrFin], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return false;
        }
        if (threadIdx.x == 0) {
            while (__hip_atomic_load(&a.gbar[kScrFin], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != (u64)gridDim.x - 1)
                __builtin_amdgcn_s_sleep(1);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        }
        __syncthreads();
        return true;
    }
    // Workgroup 0, last (every store of the call has drained: last_to_finish):
    // the call's end line (Status.fin: receive count and digest, phase stamps,
    // exit time, the sealed completion word) in ONE store of eight lanes of
    // wave 0, then scratch words [0..3] back to zero for the rank's next call
    // (so no memset precedes a launch; the next call's kernel starts only
    // after this one has retired).
    __device__ void finish_last() const {
        if (threadIdx.x >= 64) return;
        const u64 t_end = now_ticks();
        const u64 v0 = __shfl(rdone, 0, 64), v1 = __shfl(rdig, 0, 64), v2 = __shfl(ts[kTsEntry], 0, 64),
                  v3 = __shfl(ts[kTsPosted], 0, 64), v4 = __shfl(ts[kTsFirst], 0, 64), v5 = __shfl(ts[kTsLoop], 0, 64),
                  v6 = __shfl(t_end, 0, 64);
        const u64 w = fin_word(a.done_token, v0, v1, v2, v3, v4, v5, v6);
        const int l = (int)threadIdx.x;
        const u64 mine = l == 0 ? v0 : l == 1 ? v1 : l == 2 ? v2 : l == 3 ? v3 : l == 4 ? v4 : l == 5 ? v5
                                                                                         : l == 6 ? v6 : w;
        if (l < 8) st_sys(&a.status->fin.recv_done + l, mine);
        if (l == 0) {
            for (int k = 0; k < 4; ++k) __hip_atomic_store(&a.gbar[k], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&a.gbar[kScrGo], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&a.gbar[kScrReady], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }

    // ---- non-blocking check mode (k_xfer_nbcheck) ----------------------------
    // receive slot j of the rank whose rx / ring these are (ring_slot)
    __device__ unsigned char* slot_base(unsigned char* rx0, unsigned char* ring0, int j) const {
        const int s = ring_slot(j, a.iters, a.slots);
        return s == 0 ? rx0 : ring0 + (long long)(s - 1) * a.len;
    }

    // Check this workgroup's chunk of receive j: checksum + poison its slot
    // (the last receive stays in rx unpoisoned), add the chunk sum into
    // csum[j], count the chunk in cnt[j], then hand the slot back to the
    // sender (credit) — after the poison stores drained, so none can land on
    // the next payload.
    __device__ void check_nb(int j) const {
        const long long n = a.len;
        if (a.lag_ticks && (int)blockIdx.x == a.lag_wg && j + 1 == a.iters) {
            // test knob (MPX_TEST_LAG_WG): this workgroup is late to check the
            // call's last receive, so the call ends well after the peer's
            if (threadIdx.x == 0) {
                const u64 t0 = now_ticks();
                while (now_ticks() - t0 < a.lag_ticks) __builtin_amdgcn_s_sleep(127);
            }
            __syncthreads();
        }
        const u64 poison = 0x5a5a5a5a5a5a5a5aull ^ (u64)j;
        const u64 acc = sum_chunk(slot_base(a.rx, a.ring, j), n, poison, j + 1 == a.iters);
        const u64 s = block_sum(acc, lds4);
        if (threadIdx.x == 0) {
            if (s) atomicAdd(&a.csum[j], s);
            __hip_atomic_fetch_add(&a.cnt[j], 1ull, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            st_sys(&a.peer_mb->credit[a.my_slot][blockIdx.x], a.rx_seq0 + (u64)j + 1);
        }
    }

    // Wait until ready() holds (evaluated by every lane, all must agree),
    // checking — in order — every receive of this workgroup's chunk that
    // lands meanwhile.  Both sides do this whenever they wait, so a sender
    // waiting for a free slot never starves the receiver that must free it.
    template <class Ready>
    __device__ bool nb_wait(Ready ready, int* next, int iter) const {
        u64 t0 = now_ticks(), spins = 0;
        for (;;) {
            if (__syncthreads_and(ready())) return true;
            const bool landed = __syncthreads_or(
                threadIdx.x == 0 && *next < a.iters &&
                ld_sys(&a.my_mb->flag[a.peer_slot][blockIdx.x]) >= a.rx_seq0 + (u64)*next + 1);
            if (landed) {
                check_nb(*next);
                ++*next;
                t0 = now_ticks();
                continue;
            }
            if (__syncthreads_or(threadIdx.x == 0 && should_stop(++spins, t0))) {
                if (threadIdx.x == 0) give_up(iter);
                __syncthreads();
                return false;
            }
            __builtin_amdgcn_s_sleep(1);
        }
    }

    // Waitall over receives [lo, hi) (workgroup 0): each is complete once
    // every workgroup has checked its chunk; count them and add their
    // finished checksums into the digest (thread 0's registers).
    __device__ bool nb_waitall(int lo, int hi, u64* done, u64* dig, u64 fmix, int* next, int iter) const {
        const u64 want = (u64)a.nwg;
        const bool ok = nb_wait(
            [&] {
                bool r = true;
                for (int j = lo + (int)threadIdx.x; j < hi; j += kBlock)
                    r &= __hip_atomic_load(&a.cnt[j], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) >= want;
                return r;
            },
            next, iter);
        if (!ok) return false;
        u64 part = 0;
        for (int j = lo + (int)threadIdx.x; j < hi; j += kBlock)
            part += __hip_atomic_load(&a.csum[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ^ fmix;
        const u64 s = block_sum(part, lds4);
        *done += (u64)(hi - lo);
        *dig += s;
        return true;
    }

    // all workgroups finished check(): the 1-WG ack must not overtake a poison
    __device__ bool grid_sync(int iter) const {
        __syncthreads();
        if (threadIdx.x == 0) {
            __hip_atomic_fetch_add(&a.gbar[0], 1ull, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            if (blockIdx.x == 0) {
                const u64 want = (u64)gridDim.x * (u64)(iter + 1);
                const u64 t0 = now_ticks();
                u64 spins = 0;
                while (__hip_atomic_load(&a.gbar[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < want) {
                    if (should_stop(++spins, t0)) { give_up(iter); break; }
                    __builtin_amdgcn_s_sleep(1);
                }
            }
        }
        __syncthreads();
        return !aborted();
    }

    // ---- pull mode (k_xfer_pull) ---------------------------------------------
    // Bounded one-lane poll of a word this rank's workgroup reads; `sys` =
    // a word the peer writes (system scope), else a device-local counter.
    template <bool SYS>
    __device__ bool poll_ge(const u64* p, u64 want, int iter) const {
        if (threadIdx.x == 0) {
            const u64 t0 = now_ticks();
            u64 spins = 0;
            for (;;) {
                const u64 v = SYS ? ld_sys(p) : __hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
                if (v >= want) break;
                if (should_stop(++spins, t0)) { give_up(iter); break; }
                __builtin_amdgcn_s_sleep(1);
            }
        }
        __syncthreads();
        return !aborted();
    }

    // Send (workgroup 0): tx holds push `seq` — one system-scope store into
    // the peer's ready word.  tx is read-only while the loop runs and the
    // reference re-sends the same buffer every iteration (mpi_perf.c:74,80,
    // 99,105,136), so no byte moves here.  `landed` > 0: first wait until
    // that many chunks of this call's receives are in rx (a blocking Recv
    // completes before the next Send, mpi_perf.c:75-80).
    __device__ bool pull_send(u64 seq, u64 landed, int iter) const {
        if (blockIdx.x != 0) return true;
        if (landed && !poll_ge<false>(&a.gbar[kScrLanded], landed, iter)) return false;
        if (threadIdx.x == 0) st_sys(&a.peer_mb->ready[a.my_slot], seq);
        return true;
    }

    // This workgroup's chunk of a pull: units from the peer's tx into rx, 8
    // loads in flight per lane.  Loads are sc0|sc1 (system scope: each
    // iteration's bytes come from the peer's memory, not from a line this
    // GPU cached in an earlier iteration or call); stores are sc0|sc1
    // write-through, as a push lands, so check mode and the host read what
    // arrived.  Units past the chunk are out of the resources' range (loads
    // return 0, stores are dropped), so the loop has no per-unit branch.
    __device__ void pull_units(__amdgpu_buffer_rsrc_t src, __amdgpu_buffer_rsrc_t dst, int nv) const {
        constexpr int D = 8;
        for (int v = threadIdx.x; v < nv; v += D * kBlock) {
            v4u r[D];
#pragma unroll
            for (int j = 0; j < D; ++j)
                r[j] = __builtin_amdgcn_raw_buffer_load_b128(src, (unsigned)(v + j * kBlock) * 16, 0, kAuxSys);
#pragma unroll
            for (int j = 0; j < D; ++j)
                __builtin_amdgcn_raw_buffer_store_b128(r[j], dst, (unsigned)(v + j * kBlock) * 16, 0, kAuxSys);
        }
    }

    // Wait until the peer's ready word covers push `seq`.  The value last
    // read is kept in LDS (s_seen): one read that shows a later push covers
    // every push up to it, so the word is polled only when behind.
    __device__ bool wait_ready(u64 seq, int iter) const {
        if (threadIdx.x == 0 && *s_seen < seq) {
            const u64* p = &a.my_mb->ready[a.peer_slot];
            const u64 t0 = now_ticks();
            u64 spins = 0;
            for (;;) {
                const u64 v = ld_sys(p);
                if (v >= seq) { *s_seen = v; break; }
                if (should_stop(++spins, t0)) { give_up(iter); break; }
                __builtin_amdgcn_s_sleep(1);
            }
        }
        __syncthreads();
        return !aborted();
    }

    // Receive (every workgroup, grid = nwg): wait for the peer's ready word,
    // load this workgroup's chunk of the peer's tx into rx, check it (check
    // mode).  `publish` > 0: then drain, return the chunk to the peer (credit
    // = seq: its tx chunk may change again, for every push up to seq) and
    // count `publish` receives of this workgroup landed.  The non-blocking
    // loop publishes every nb_publish receives (and at the last): the others
    // are loads and stores only, with no drain between them.
    __device__ bool pull_recv(long long n, u64 seq, int iter, u64 publish = 1) const {
        if (!wait_ready(seq, iter)) return false;
        // system-scope acquire (buffer_inv sc0 sc1: the L2's lines of
        // non-local memory, i.e. a peer GPU's tx, are dropped, so every
        // iteration's loads cross the link), completed before any wave loads
        // (every wave drains; draining only the fencing wave read the same:
        // profiles/r03_pull_publish_ab.jsonl)
        if (threadIdx.x == 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
        drain_stores();
        __syncthreads();
        if (a.lag_ticks && (int)blockIdx.x == a.lag_wg && iter + 1 == a.iters) {
            // test knob (MPX_TEST_LAG_WG): this workgroup is late to load the
            // call's last payload, so the peer's call must wait for it
            if (threadIdx.x == 0) {
                const u64 t0 = now_ticks();
                while (now_ticks() - t0 < a.lag_ticks) __builtin_amdgcn_s_sleep(127);
            }
            __syncthreads();
        }
        long long lo, hi;
        chunk_of(n, &lo, &hi);
        if (lo < hi) {
            const unsigned bytes = (unsigned)(hi - lo);
            const __amdgpu_buffer_rsrc_t src = rsrc(a.peer_tx + lo, bytes);
            const __amdgpu_buffer_rsrc_t dst = rsrc(a.rx + lo, bytes);
            const int nv = (int)(bytes >> 4);
            if (a.skip_push != iter + 1) {             // test knob: this payload is "lost"
                pull_units(src, dst, nv);
                const unsigned tail = bytes & 15;
                if (threadIdx.x < tail) {
                    const unsigned o = (unsigned)nv * 16 + threadIdx.x;
                    __builtin_amdgcn_raw_buffer_store_b8(__builtin_amdgcn_raw_buffer_load_b8(src, o, 0, kAuxSys), dst, o,
                                                         0, kAuxSys);
                }
            }
        }
        if (a.check) check(n, iter);                   // (drains first: sum_chunk)
        if (!publish) return true;
        drain_stores();                                // loads and stores of every wave
        __syncthreads();
        if (threadIdx.x == 0) {
            st_sys(&a.peer_mb->credit[a.my_slot][wg()], seq);
            __hip_atomic_fetch_add(&a.gbar[kScrLanded], publish, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        }
        return true;
    }

    // Workgroup 0: every chunk of this side's sends up to `seq` was loaded
    // by the peer (its credits), so tx may change once the call returns —
    // MPI_Send's buffer-reuse rule, and the non-blocking loop's Waitall over
    // the send requests (mpi_perf.c:110,122).
    __device__ bool wait_pulled(u64 seq, int iter) const {
        if (blockIdx.x != 0) return true;
        if (threadIdx.x < 64) {
            const u64* c = &a.my_mb->credit[a.peer_slot][0];
            const u64 t0 = now_ticks();
            u64 spins = 0;
            for (;;) {
                bool ok = true;
                for (int j = threadIdx.x; j < a.nwg; j += 64) ok &= ld_sys(c + j) >= seq;
                if (__all(ok)) break;
                if (should_stop(++spins, t0)) {
                    if (threadIdx.x == 0) give_up(iter);
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
            }
        }
        __syncthreads();
        return !aborted();
    }
};

// ---------------------------------------------------------------------------
// Per-iteration latency recorder (mpx_lat_*, LatBlock): the blocking loops'
// traced instantiations (k_xfer_lat, k_xfer_pull_lat).  Lane 0 of workgroup
// 0 reads the clock once at the bottom of every iteration — where the
// untraced loop stamps kTsFirst at i = 0, and for i = 0 that read IS the
// kTsFirst stamp — and streams d = t[i+1] - t[i] into registers (min, max,
// the iteration of the first maximum; the sum telescopes), one no-return
// atomic add on its histogram bucket and, while i < raw_cap, one plain store
// of the stamp: no load of the recorder stands in the loop.  Behind the
// call's finish barrier it folds the registers into the rank's block (a plain
// read-modify-write: a rank runs one call at a time, and the host touches
// the block only between calls, on the rank's stream).
// LatTrace<false> is empty: the untraced kernels read no clock for it.
// ---------------------------------------------------------------------------
// The clock read and its wait as ONE statement, fenced from the scheduler.
__device__ __forceinline__ u64 lat_stamp() {
    u64 t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}

// ANYWG: lane 0 of EVERY workgroup traces, into a block of its workgroup's own
// (k_xfer_fan_ll<., true>: workgroup k is link k); false: workgroup 0's lane 0 only.
template <bool LAT, bool ANYWG = false>
struct LatTrace {
    __device__ bool on() const { return false; }
    __device__ void begin(LatBlock*, u64, u64, int) {}
    __device__ u64 tick(int) { return 0; }
    __device__ void end() {}
};
template <bool ANYWG>
struct LatTrace<true, ANYWG> {
    LatBlock* blk = nullptr;
    u64 prev = 0, mn = ~0ull, mx = 0;   // (the sum telescopes: prev - t[0], taken at the end)
    unsigned cap = 0, maxi = 0, n = 0;

    __device__ bool on() const { return (ANYWG || blockIdx.x == 0) && threadIdx.x == 0; }
    // t[0]: the instant mpx_phases.first_iter_s counts from (complete_call's
    // t_go): the peer's post on a side that pushes first, else the entry
    __device__ __forceinline__ void begin(LatBlock* b, u64 t_entry, u64 t_posted, int iters) {
        if (!on()) return;
        blk = b;
        prev = t_posted >= t_entry ? t_posted : t_entry;
        // raw[] holds raw_cap + 1 stamps (lat_block_bytes): slot 0 here, slot
        // i + 1 only while i < cap <= raw_cap (tick) — the one bound
        const u64 rc = b->raw_cap;
        cap = (u64)iters < rc ? (unsigned)iters : (unsigned)rc;
        b->raw[0] = prev;
    }
    // the end of iteration i
    __device__ __forceinline__ u64 tick(int i) {
        const u64 t = lat_stamp();
        const u64 d = t - prev;
        prev = t;
        if (d < mn) mn = d;
        if (d > mx) {
            mx = d;
            maxi = (unsigned)i;
        }
        ++n;
        __hip_atomic_fetch_add(&blk->hist[mpx_lat_bucket(d)], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((unsigned)i < cap) blk->raw[(unsigned)i + 1] = t;
        return t;
    }
    __device__ __forceinline__ void end() {
        if (!on()) return;
        LatBlock& b = *blk;
        const u64 c0 = b.count;
        if (n) {
            if (c0 == 0 || mn < b.min_ticks) b.min_ticks = mn;
            if (c0 == 0 || mx > b.max_ticks) {
                b.max_ticks = mx;
                b.max_iter = maxi;
            }
            b.sum_ticks += prev - b.raw[0];
            b.count = c0 + n;
        }
        b.calls += 1;
        b.last_iters = n;
        b.raw_n = 1 + (u64)(n < cap ? n : cap);
    }
};

// One instantiation per (mode, side): each carries only its own loop, so
// register pressure stays within 4 waves per SIMD (<= 128 VGPRs, no spills)
// and four k_xfer workgroups fit on a CU — pairs that share one GPU
// (loopback ranks, -g maps) keep every workgroup resident.  LAT: the traced
// form (LatTrace); k_xfer is the LAT = false wrapper, k_xfer_lat the other.
// The arguments come by value: the pull kernels then compile to the
// instructions they had as kernels of their own, and the pushing sides load
// their arguments once instead of at every use.
template <int MODE, int GROUP, bool LAT, bool SEQ = false>
__device__ __forceinline__ void xfer_body(const XferArgs a) {
    __shared__ int s_abort;
    __shared__ u64 lds4[4];
    extern __shared__ v4u s_tx[];            // a.stage: dynamic LDS = one chunk
    if (threadIdx.x == 0) s_abort = 0;
    Loop<MODE, false, SEQ> L{a, &s_abort, lds4, s_tx, {}};
    LatTrace<LAT> T;
    if (!L.wait_go()) {
        if (L.last_to_finish()) L.finish_last();
        return;
    }
    L.stamp(kTsEntry);
    const long long n = a.len;
    // the size this side sends: B, or the 1-byte ack of unidir group 0
    const long long send_len = (MODE == MPX_MODE_UNIDIR && GROUP == 0) ? 1 : n;
    const bool ll_send = blockIdx.x == 0 && L.is_ll(send_len);
    if constexpr (!SEQ) {
        if (ll_send) L.preload_ll(send_len);
    }
    u64 txs = a.tx_seq0, rxs = a.rx_seq0;
    u64 done = 0;                                       // receives completed (Status.recv_done)
    int inflight = 0;
    L.post_receives();
    // A side whose first action is a push waits for the peer's post.  Group 0
    // of ping-pong / unidir pushes only after its first receive, which the
    // peer sent after it saw this side's post, so its peer has started too.
    constexpr bool push_first = MODE == MPX_MODE_NONBLOCKING || GROUP == 1;
    const bool go = !push_first || a.iters == 0 || L.wait_posted();
    if constexpr (LAT) T.begin(a.lat, L.ts[kTsEntry], L.ts[kTsPosted], a.iters);
    // Group 1's last receive (ping-pong, unidir) without check mode: only
    // workgroup 0 waits for it (it counts receives and ends the call); the
    // others have nothing left to do once their last push is out, so they
    // leave, and their finish count is in before workgroup 0 needs it.
    const bool last_recv_wg0 = !a.check && blockIdx.x != 0;
    for (int i = 0; go && i < a.iters; ++i) {
        const bool skip = a.skip_push == i + 1;        // test knob only
        // SEQ: this iteration's key, scalar; an LL send's units are generated
        // here, ahead of whatever this side waits for first
        u64 key = 0;
        if constexpr (SEQ) {
            key = a.seq_tx_key ^ ((u64)(unsigned)i << 24);
            if (ll_send && !skip) L.gen_ll(send_len, key);
        }
        if constexpr (MODE == MPX_MODE_PINGPONG) {    // mpi_perf.c:70-82
            if constexpr (GROUP == 1) {
                L.send(n, ++txs, skip, key);           // Send(tx, B, tag 1)
                if (i + 1 == a.iters && last_recv_wg0) break;
                if (!L.recv(n, ++rxs, i)) break;       // Recv(rx, B, tag 2)
                ++done;
                if (a.check) L.check(n, i);
            } else {
                if (!L.recv(n, ++rxs, i)) break;       // Recv(rx, B, tag 1)
                ++done;
                if (a.check) L.check(n, i);
                L.send(n, ++txs, skip, key);           // Send(tx, B, tag 2)
            }
        } else if constexpr (MODE == MPX_MODE_UNIDIR) {  // mpi_perf.c:132-144
            if constexpr (GROUP == 1) {
                L.send(n, ++txs, skip, key);           // Send(tx, B)
                if (i + 1 == a.iters && last_recv_wg0) break;
                if (!L.recv(1, ++rxs, i)) break;       // Recv(rx, 1) — the ack
                ++done;
                if (a.check) L.check(1, i);
            } else {
                if (!L.recv(n, ++rxs, i)) break;       // Recv(rx, B)
                ++done;
                if (a.check) { L.check(n, i); if (!L.grid_sync(i)) break; }
                L.send(1, ++txs, skip, key);           // Send(tx, 1)
            }
        } else {                                       // mpi_perf.c:95-124
            // Isend + Irecv, slot `inflight`.  A receiver waits only at the
            // window flush (i = 255 mod 256) and at the end, so a push needs
            // its drain + flag only every a.nb_publish iterations (a divisor
            // of 256), at slot 254 (the last receive a flush waits for) and
            // at the last one: the drain's link round trip is paid once per
            // nb_publish pushes instead of once per push, and no flush waits
            // for the slot-255 push the reference leaves pending.
            const int slot = i % kNbWindow;
            L.push_bulk(n, ++txs, (i + 1) % a.nb_publish == 0 || slot == kNbWindow - 2 || i + 1 == a.iters,
                        nullptr, skip, key);
            if (inflight == kNbWindow - 1) {
                // Waitall(255, ...): receives of slots 0..254 (iterations
                // i-255 .. i-1); the receive posted in slot 255 (this
                // iteration) is not among them (mpi_perf.c:110-111)
                if (!L.wait_bulk(rxs + i, i)) break;
                done += (u64)inflight;
                inflight = 0;
            } else {
                ++inflight;
            }
        }
        // the end of a blocking iteration (the breaks above leave the loop)
        if constexpr (MODE != MPX_MODE_NONBLOCKING) {
            if constexpr (LAT) {                       // one clock read: the iteration's end, and
                if (T.on()) {                          // for i = 0 also the kTsFirst stamp
                    const u64 t = T.tick(i);
                    if (i == 0) L.ts[kTsFirst] = t;
                }
            } else if (i == 0) {
                L.stamp(kTsFirst);
            }
        }
    }
    L.stamp(kTsLoop);
    if constexpr (MODE == MPX_MODE_NONBLOCKING) {
        if (inflight > 0 && !L.aborted() && L.wait_bulk(rxs + a.iters, a.iters - 1))   // final Waitall(inflight)
            done += (u64)inflight;
        if (blockIdx.x == 0 && threadIdx.x == 0) L.rdone = done;
        if (L.last_to_finish()) L.finish_last();
    } else if (L.last_to_finish()) {
        L.account(done, (MODE == MPX_MODE_UNIDIR && GROUP == 1) ? 1 : n);
        // (folded here, not right after the loop: there the traced ping-pong
        // kernels came out with a 36-byte stack frame)
        if constexpr (LAT) T.end();
        L.finish_last();
    }
}
template <int MODE, int GROUP>
__global__ __launch_bounds__(kBlock, 4) void k_xfer(XferArgs a) {
    xfer_body<MODE, GROUP, false>(a);
}
// ping-pong and unidir only (launch_xfer): the non-blocking loop's iterations
// have no blocking step to time
template <int MODE, int GROUP>
__global__ __launch_bounds__(kBlock, 4) void k_xfer_lat(XferArgs a) {
    xfer_body<MODE, GROUP, true>(a);
}
// mpx_xfer_seq: the same loops with every pushed payload generated from the
// iteration's key (Loop's SEQ policy); never traced
template <int MODE, int GROUP>
__global__ __launch_bounds__(kBlock, 4) void k_xfer_seq(XferArgs a) {
    xfer_body<MODE, GROUP, false, true>(a);
}

// The non-blocking loop in check mode (mpi_perf.c:95-124 with every payload
// checksummed).  The reference posts up to 256 receives into ONE rx
// (:100,104); here every receive lands in a slot of its own (ring_slot), so
// each payload can be checksummed before anything overwrites it.  A sender
// reuses a slot only after the receiver handed it back (Mailbox.credit);
// every wait checks the receives that land meanwhile, so neither side can
// starve the other.  Each workgroup pushes and checks its own chunk.  The
// windowing is the reference's: Waitall(255) at slot 255 over slots 0..254,
// the final Waitall(inflight); workgroup 0 counts exactly those receives and
// digests their checksums.  The receives the reference leaves pending (slot
// 255 of each full window) are still checked — every payload is — but not
// counted.  Grid = a.nwg; all workgroups push B bytes.
__global__ __launch_bounds__(kBlock, 4) void k_xfer_nbcheck(XferArgs a) {
    __shared__ int s_abort;
    __shared__ u64 lds4[4];
    extern __shared__ v4u s_tx[];
    if (threadIdx.x == 0) s_abort = 0;
    Loop<MPX_MODE_NONBLOCKING> L{a, &s_abort, lds4, s_tx, {}};
    if (!L.wait_go()) {
        if (L.last_to_finish()) L.finish_last();
        return;
    }
    L.stamp(kTsEntry);
    const long long n = a.len;
    const int w = blockIdx.x;
    const u64 fmix = mix64((u64)n);
    const u64* credit = &a.my_mb->credit[a.peer_slot][w];
    int next = 0, inflight = 0;
    u64 done = 0, dig = 0;
    // The peer's receive slots are free for this call only once the peer's
    // kernel of this call runs (Mailbox.posted): its previous kernel — every
    // workgroup's checks and poison stores of the previous call, whatever
    // that call's length, width and slot layout — has finished by then.
    // Credits alone cannot say so: they are per workgroup, and the previous
    // call's last credits already satisfy this call's first S pushes.
    L.post_receives();
    bool ok = a.iters == 0 || L.nb_wait([&] { return threadIdx.x != 0 || L.peer_posted(); }, &next, 0);
    L.stamp(kTsPosted);
    for (int i = 0; i < a.iters && ok; ++i) {
        // slot ring_slot(i) was last used by push i - S of this call: wait
        // for its credit
        if (i >= a.slots) {
            const u64 want = a.tx_seq0 + (u64)(i - a.slots + 1);
            ok = L.nb_wait([&] { return threadIdx.x != 0 || ld_sys(credit) >= want; }, &next, i);
            if (!ok) break;
        }
        L.push_bulk(n, a.tx_seq0 + (u64)i + 1, true, L.slot_base(a.peer_rx, a.peer_ring, i), a.skip_push == i + 1);
        if (inflight == kNbWindow - 1) {               // Waitall(255): iterations i-255 .. i-1
            ok = L.nb_wait([&] { return next >= i; }, &next, i);
            if (ok && w == 0) ok = L.nb_waitall(i - inflight, i, &done, &dig, fmix, &next, i);
            inflight = 0;
        } else {
            ++inflight;
        }
    }
    if (ok && inflight > 0) {                          // Waitall(inflight)
        ok = L.nb_wait([&] { return next >= a.iters; }, &next, a.iters - 1);
        if (ok && w == 0) ok = L.nb_waitall(a.iters - inflight, a.iters, &done, &dig, fmix, &next, a.iters - 1);
    }
    // every payload: also the receives the reference leaves pending
    if (ok) L.nb_wait([&] { return next >= a.iters; }, &next, a.iters - 1);
    if (w == 0 && threadIdx.x == 0) {
        L.rdone = done;
        L.rdig = dig;
    }
    if (L.last_to_finish()) L.finish_last();
}

// k_xfer_seq_nbcheck: k_xfer_nbcheck with every push generated from its
// iteration's key (mpx_xfer_seq; Loop's SEQ policy) — the same waits, slots,
// credits, windows and accounting, line for line.  A kernel of its own: with
// the loop shared through an inlined function, k_xfer_nbcheck came out with
// other SGPR spills (44 -> 46) than it has as a kernel written out.
__global__ __launch_bounds__(kBlock, 4) void k_xfer_seq_nbcheck(XferArgs a) {
    __shared__ int s_abort;
    __shared__ u64 lds4[4];
    extern __shared__ v4u s_tx[];
    if (threadIdx.x == 0) s_abort = 0;
    Loop<MPX_MODE_NONBLOCKING, false, true> L{a, &s_abort, lds4, s_tx, {}};
    if (!L.wait_go()) {
        if (L.last_to_finish()) L.finish_last();
        return;
    }
    L.stamp(kTsEntry);
    const long long n = a.len;
    const int w = blockIdx.x;
    const u64 fmix = mix64((u64)n);
    const u64* credit = &a.my_mb->credit[a.peer_slot][w];
    int next = 0, inflight = 0;
    u64 done = 0, dig = 0;
    L.post_receives();
    bool ok = a.iters == 0 || L.nb_wait([&] { return threadIdx.x != 0 || L.peer_posted(); }, &next, 0);
    L.stamp(kTsPosted);
    for (int i = 0; i < a.iters && ok; ++i) {
        // slot ring_slot(i) was last used by push i - S of this call: wait
        // for its credit
        if (i >= a.slots) {
            const u64 want = a.tx_seq0 + (u64)(i - a.slots + 1);
            ok = L.nb_wait([&] { return threadIdx.x != 0 || ld_sys(credit) >= want; }, &next, i);
            if (!ok) break;
        }
        L.push_bulk(n, a.tx_seq0 + (u64)i + 1, true, L.slot_base(a.peer_rx, a.peer_ring, i), a.skip_push == i + 1,
                    a.seq_tx_key ^ ((u64)(unsigned)i << 24));
        if (inflight == kNbWindow - 1) {               // Waitall(255): iterations i-255 .. i-1
            ok = L.nb_wait([&] { return next >= i; }, &next, i);
            if (ok && w == 0) ok = L.nb_waitall(i - inflight, i, &done, &dig, fmix, &next, i);
            inflight = 0;
        } else {
            ++inflight;
        }
    }
    if (ok && inflight > 0) {                          // Waitall(inflight)
        ok = L.nb_wait([&] { return next >= a.iters; }, &next, a.iters - 1);
        if (ok && w == 0) ok = L.nb_waitall(a.iters - inflight, a.iters, &done, &dig, fmix, &next, a.iters - 1);
    }
    // every payload: also the receives the reference leaves pending
    if (ok) L.nb_wait([&] { return next >= a.iters; }, &next, a.iters - 1);
    if (w == 0 && threadIdx.x == 0) {
        L.rdone = done;
        L.rdig = dig;
    }
    if (L.last_to_finish()) L.finish_last();
}

// k_xfer_pull: the three loops with every B-byte payload PULLED by its
// receiver (MPX_XFER_PULL; SURVEY.md §7 step 4, "try pull as well").  A send
// is one store into the peer's ready word (Loop::pull_send); the receiver's
// workgroups load their chunks of the sender's tx over xGMI into their own rx
// (Loop::pull_recv).  A receive is complete once every workgroup's chunk
// is in (the local landed counter); the sender's tx is free again once every
// chunk's credit came back, which each sending side waits for before its
// kernel ends.  rx is only ever written by its own rank's kernel, so no
// payload of the next call can land before this rank's next call starts.
// LL messages stay pushes (their data is their flag), and so does the
// unidir 1-byte ack (mpi_perf.c:137,142).  Grid: nwg for a side that
// receives B-byte payloads, 1 for unidir group 1 (it only publishes and
// takes acks).
// LAT: the traced form (LatTrace), which also takes the kTsFirst and kTsLoop
// stamps the untraced pull loop does not (mpx_phases.first_iter_s, tail_s).
template <int MODE, int GROUP, bool LAT>
__device__ __forceinline__ void xfer_pull_body(const XferArgs a) {
    __shared__ int s_abort;
    __shared__ u64 lds4[4];
    __shared__ u64 s_seen;
    if (threadIdx.x == 0) {
        s_abort = 0;
        s_seen = 0;
    }
    Loop<MODE> L{a, &s_abort, lds4, nullptr, {}, &s_seen};
    LatTrace<LAT> T;
    if (!L.wait_go()) {
        if (L.last_to_finish()) L.finish_last();
        return;
    }
    L.stamp(kTsEntry);
    const long long n = a.len;
    const u64 nw = (u64)a.nwg;
    if (MODE == MPX_MODE_UNIDIR && GROUP == 0 && blockIdx.x == 0) L.preload_ll(1);   // the ack's byte
    __syncthreads();
    u64 txs = a.tx_seq0, rxs = a.rx_seq0, done = 0, pending = 0;
    L.post_receives();
    bool ok = true;
    int inflight = 0;
    if constexpr (LAT) T.begin(a.lat, L.ts[kTsEntry], L.ts[kTsPosted], a.iters);
    for (int i = 0; ok && i < a.iters; ++i) {
        if constexpr (MODE == MPX_MODE_PINGPONG) {    // mpi_perf.c:70-82
            if constexpr (GROUP == 1) {
                ok = L.pull_send(++txs, nw * (u64)i, i) && L.pull_recv(n, ++rxs, i);   // Send(tag 1), Recv(tag 2)
            } else {
                ok = L.pull_recv(n, ++rxs, i) && L.pull_send(++txs, nw * (u64)(i + 1), i);   // Recv(tag 1), Send(tag 2)
            }
            if (ok) ++done;
        } else if constexpr (MODE == MPX_MODE_UNIDIR) {  // mpi_perf.c:132-144
            if constexpr (GROUP == 1) {
                ok = L.pull_send(++txs, 0, i) && L.recv(1, ++rxs, i);   // Send(tx, B), Recv(rx, 1)
                if (ok) {
                    ++done;
                    if (a.check) L.check(1, i);
                }
            } else {
                ok = L.pull_recv(n, ++rxs, i);           // Recv(rx, B)
                if (ok) ++done;
                // Send(tx, 1) once every chunk is in (workgroup 0's LL push)
                if (ok && blockIdx.x == 0) ok = L.template poll_ge<false>(&a.gbar[kScrLanded], nw * (u64)(i + 1), i);
                if (ok) L.send(1, ++txs);
            }
        } else {                                       // mpi_perf.c:95-124
            // Isend + Irecv, slot `inflight`; the receive is published (drain,
            // credit, landed count) every nb_publish receives and at the last
            // one — kNbWindow is a multiple of nb_publish, so slot 255 (the
            // flush) is always a publish point
            ++pending;
            const bool pub = (i + 1) % a.nb_publish == 0 || i + 1 == a.iters;
            ok = L.pull_send(++txs, 0, i) && L.pull_recv(n, ++rxs, i, pub ? pending : 0);
            if (pub) pending = 0;
            if (ok && inflight == kNbWindow - 1) {
                // Waitall(255): every workgroup waits until all chunks of
                // receives 0..i are in (so none runs into the next window
                // ahead of the count), workgroup 0 for the peer's loads of
                // sends 0..254 (iterations i-255 .. i-1)
                ok = L.template poll_ge<false>(&a.gbar[kScrLanded], nw * (u64)(i + 1), i) && L.wait_pulled(txs - 1, i);
                done += (u64)inflight;
                inflight = 0;
            } else {
                ++inflight;
            }
        }
        if constexpr (LAT) {                           // the iteration's end on workgroup 0
            if (ok && T.on()) {
                const u64 t = T.tick(i);
                if (i == 0) L.ts[kTsFirst] = t;
            }
        }
    }
    if constexpr (LAT) L.stamp(kTsLoop);
    // every send of the call loaded by the peer before tx may change again
    const bool sent_bulk = MODE != MPX_MODE_UNIDIR || GROUP == 1;
    if (ok && sent_bulk && a.iters > 0 && !a.no_pull_wait) ok = L.wait_pulled(txs, a.iters - 1);
    if constexpr (MODE == MPX_MODE_NONBLOCKING) {
        // final Waitall(inflight); then workgroup 0 counts and digests the
        // receives the reference waits for (all but slot 255 of each full
        // window)
        if (blockIdx.x == 0) {
            if (ok && a.iters > 0) ok = L.template poll_ge<false>(&a.gbar[kScrLanded], nw * (u64)a.iters, a.iters - 1);
            if (ok) done += (u64)inflight;
            u64 part = 0;
            if (ok && a.check) {
                const u64 fmix = mix64((u64)n);
                for (int j = threadIdx.x; j < a.iters; j += kBlock)
                    if (j % kNbWindow != kNbWindow - 1)
                        part += __hip_atomic_load(&a.csum[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ^ fmix;
            }
            const u64 s = block_sum(part, lds4);
            if (threadIdx.x == 0) {
                L.rdone = done;
                L.rdig = s;
            }
        }
        if (L.last_to_finish()) L.finish_last();
    } else if (L.last_to_finish()) {
        L.account(done, (MODE == MPX_MODE_UNIDIR && GROUP == 1) ? 1 : n);
        if constexpr (LAT) T.end();
        L.finish_last();
    }
}
template <int MODE, int GROUP>
__global__ __launch_bounds__(kBlock, 4) void k_xfer_pull(XferArgs a) {
    xfer_pull_body<MODE, GROUP, false>(a);
}
template <int MODE, int GROUP>
__global__ __launch_bounds__(kBlock, 4) void k_xfer_pull_lat(XferArgs a) {
    xfer_pull_body<MODE, GROUP, true>(a);
}

// ---------------------------------------------------------------------------
// k_xfer_hostlink: a GPU rank's side of the ping-pong or unidir loop with a
// CPU endpoint (mpx_xfer_hostlink; the endpoint's side is mpx_hostlink.h's
// run()).  The endpoint cannot write device memory, so every shared word and
// byte is in pinned host memory and this kernel does all the moving:
//   a.peer_mb  the endpoint's `in` box   (this rank writes: flag, ll, credit, posted)
//   a.my_mb    the endpoint's `out` box  (this rank polls across the link: ll, ready, posted)
//   a.peer_rx / a.peer_tx  the endpoint's rx / tx;  a.my_slot = a.peer_slot = this rank
// Both boxes have the device mailbox's layout, so the sends are the pair
// loops' own (Loop::push_ll, push_bulk: sc0 sc1 payload stores, every wave's
// drain, then the flag) and so are the receives' bodies (Loop::wait_ll's
// granule poll and unpack; Loop::pull_recv's chunk loads from the endpoint's
// tx, check, credit).  What is new is who reads host memory while waiting:
// only workgroup 0.  It polls the endpoint's word (posted, ready, or the LL
// row) and republishes what it saw in a device scratch word (kScrHostPosted;
// kScrHostSeen = receives of this call seen so far), which the other
// workgroups poll at agent scope — as wait_go hands the host's go word on in
// kScrGo — so that up to 255 pollers of one host line do not share the link
// with the payload loads (a supposition, not a measurement: DESIGN.md §5).
// Grid: 1 when both directions are LL, else a.nwg; co-resident (4 per CU).
// ---------------------------------------------------------------------------
// LAT: the traced form (mpx_hostlink_lat_*; LatTrace, workgroup 0's lane 0)
// into a.lat, the block of the endpoint's rank in the rank's host-link
// recorder.  t[0] is the instant first_iter_s counts from (kTsPosted on the
// side that pushes first, else kTsEntry); the one clock read at the bottom of
// iteration i is t[i+1] and, for i = 0, the kTsFirst stamp.  k_xfer_hostlink
// is the LAT = false wrapper, k_hostlink_lat the other.
// SEQ: a sequenced call (mpx_xfer_hostlink_seq; Loop's SEQ policy): every send
// is generated in registers from its iteration's key, a.seq_tx_key ^ i << 24 —
// an LL send's units by gen_ll in place of the one preload_ll, a bulk send's
// by push_bulk's generating branch — so tx is never read and nothing is
// staged in LDS (a.stage = 0).  The receives are the same code: what they
// must find is the caller's to say (check_verdict's per-payload form).
// k_hostlink_gen is that wrapper; there is no traced form.
template <int MODE, int GROUP, bool LAT, bool SEQ = false>
__device__ __forceinline__ void hostlink_body(const XferArgs a) {
    static_assert(MODE == MPX_MODE_PINGPONG || MODE == MPX_MODE_UNIDIR, "the blocking loops only");
    // statics of 48 bytes: the dynamic region (the staged tx chunk) stays 16-byte aligned
    __shared__ __attribute__((aligned(16))) u64 s_w[6];   // block_sum's four, s_seen, s_abort
    extern __shared__ v4u s_tx[];
    int* s_abort = reinterpret_cast<int*>(&s_w[5]);
    if (threadIdx.x == 0) {
        *s_abort = 0;
        s_w[4] = 0;
    }
    __syncthreads();
    Loop<MODE, false, SEQ> L{a, s_abort, s_w, s_tx, {}, &s_w[4]};
    L.stamp(kTsEntry);
    const long long n = a.len;
    constexpr bool sends_n = MODE != MPX_MODE_UNIDIR || GROUP == 1;   // else the 1-byte ack
    constexpr bool recvs_n = MODE != MPX_MODE_UNIDIR || GROUP == 0;
    const long long send_len = sends_n ? n : 1, recv_len = recvs_n ? n : 1;
    const bool ll_send = L.is_ll(send_len), ll_recv = L.is_ll(recv_len);
    const bool wg0 = blockIdx.x == 0;
    if constexpr (!SEQ) {
        if (wg0 && ll_send) L.preload_ll(send_len);
    }
    u64 txs = a.tx_seq0, rxs = a.rx_seq0, done = 0;
    // workgroup 0 saw it in host memory: tell the others; they wait for that
    auto relay = [&](int word, u64 v) {
        if (threadIdx.x == 0 && gridDim.x > 1)
            __hip_atomic_store(&a.gbar[word], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    LatTrace<LAT> T;
    L.post_receives();
    bool ok = true;
    if (GROUP == 1 && a.iters > 0) {
        // this side pushes first: the endpoint's receives of this call are posted
        if (wg0) {
            ok = L.template poll_ge<true>(&a.my_mb->posted[a.peer_slot], a.call, 0);
            if (ok) relay(kScrHostPosted, 1);
        } else {
            ok = L.template poll_ge<false>(&a.gbar[kScrHostPosted], 1, 0);
        }
        L.stamp(kTsPosted);
    }
    if constexpr (LAT) T.begin(a.lat, L.ts[kTsEntry], L.ts[kTsPosted], a.iters);
    auto send = [&](int i) {
        ++txs;
        const bool lose = sends_n && a.skip_push == i + 1;   // test knob: a B-byte payload, never an ack
        // SEQ: this iteration's key, scalar; an LL send's units (the ack's one
        // byte too) are generated here, ahead of the wait for the landed chunks
        u64 key = 0;
        if constexpr (SEQ) {
            key = a.seq_tx_key ^ ((u64)(unsigned)i << 24);
            if (wg0 && ll_send && !lose) L.gen_ll(send_len, key);
        }
        if (ll_send) {
            // a side that received a bulk payload answers once every chunk is in:
            // the chunks of the receives it has completed — i + 1 of them where it
            // receives first, i where it sends first (none before its first send:
            // the 0-byte unidir payload with a bulk ack, MPX_HOSTLINK_LL=0)
            const u64 landed = (u64)a.nwg * (u64)(GROUP == 1 ? i : i + 1);
            if (!ll_recv && wg0 && landed && !L.template poll_ge<false>(&a.gbar[kScrLanded], landed, i)) return false;
            if (!lose) L.push_ll(send_len, txs);
            else L.push_ll_tags_only(send_len, txs);
        } else {
            L.push_bulk(send_len, txs, true, nullptr, lose, key);
        }
        return true;
    };
    auto recv = [&](int i) {
        ++rxs;
        if (ll_recv) {
            // the granules are in the endpoint's out row: workgroup 0 polls them across the link
            if (wg0) {
                if (!L.wait_ll(recv_len, rxs, i)) return false;
                relay(kScrHostSeen, (u64)(i + 1));
                if (a.check) L.check(recv_len, i);
            } else if (!L.template poll_ge<false>(&a.gbar[kScrHostSeen], (u64)(i + 1), i)) {
                return false;
            }
        } else {
            // "tx holds message rxs": workgroup 0 reads the word, every workgroup pulls its chunk
            if (wg0) {
                if (!L.template poll_ge<true>(&a.my_mb->ready[a.peer_slot], rxs, i)) return false;
                relay(kScrHostSeen, (u64)(i + 1));
            } else if (!L.template poll_ge<false>(&a.gbar[kScrHostSeen], (u64)(i + 1), i)) {
                return false;
            }
            if (threadIdx.x == 0) s_w[4] = rxs;          // (pull_recv's own wait finds the word seen)
            __syncthreads();
            if (!L.pull_recv(recv_len, rxs, i)) return false;
        }
        ++done;
        return true;
    };
    for (int i = 0; ok && i < a.iters; ++i) {
        if constexpr (GROUP == 1) ok = send(i) && recv(i);   // mpi_perf.c:72-75, 135-137
        else ok = recv(i) && send(i);                        // mpi_perf.c:79-80, 141-142
        if constexpr (LAT) {                                 // one clock read: the iteration's end, and
            if (T.on()) {                                    // for i = 0 also the kTsFirst stamp
                const u64 t = T.tick(i);
                if (i == 0) L.ts[kTsFirst] = t;
            }
        } else if (i == 0) {
            L.stamp(kTsFirst);
        }
    }
    L.stamp(kTsLoop);
    if (L.last_to_finish()) {
        L.account(done, recv_len);
        if (threadIdx.x == 0) {   // every other workgroup is done with the relay words
            __hip_atomic_store(&a.gbar[kScrHostSeen], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&a.gbar[kScrHostPosted], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if constexpr (LAT) T.end();   // (behind the finish barrier, as xfer_body folds)
        L.finish_last();
    }
}
template <int MODE, int GROUP>
__global__ __launch_bounds__(kBlock, 4) void k_xfer_hostlink(XferArgs a) {
    hostlink_body<MODE, GROUP, false>(a);
}
template <int MODE, int GROUP>
__global__ __launch_bounds__(kBlock, 4) void k_hostlink_lat(XferArgs a) {
    hostlink_body<MODE, GROUP, true>(a);
}
// mpx_xfer_hostlink_seq: the same loop with every pushed payload generated
// from its iteration's key; never traced
template <int MODE, int GROUP>
__global__ __launch_bounds__(kBlock, 4) void k_hostlink_gen(XferArgs a) {
    hostlink_body<MODE, GROUP, false, true>(a);
}

// ---------------------------------------------------------------------------
// k_hostlink_duplex: a GPU rank's side of the non-blocking loop (mpi_perf.c:
// 85-125) with a CPU endpoint (mpx_xfer_hostlink_duplex; the endpoint's side
// is mpx_hostlink.h's run_duplex()) — both directions of the PCIe link loaded
// at once.  The boxes, slots and buffers are k_xfer_hostlink's.
//   Grid: 2 * a.nwg workgroups.  The first a.nwg PUSH (Isend i: chunk w of tx
// into the endpoint's rx, Loop::push_bulk with the non-blocking loop's
// deferred publish), the other a.nwg PULL (Irecv i: chunk w of the endpoint's
// tx into rx once its ready word covers push i, Loop::pull_recv with deferred
// publish).  Posted stores and link-crossing loads so come from different
// workgroups and neither half waits for the other, except where the
// reference's loop does: at the window flush and at the end.  Loop's ANYWG
// form maps a workgroup to its chunk (wg_ = its index within its half).
//   Who reads host memory: one workgroup per direction, the first of each
// half.  The pushing half's polls the endpoint's post and, in check mode, its
// credit word; the pulling half's its ready word.  Each republishes what it
// saw in a device scratch word (kScrHostPosted, kScrHostCredit, kScrHostSeen:
// the word's value as read) for the rest of its half, and every workgroup
// keeps the highest value it has seen in LDS: an endpoint that has posted a
// whole window is polled once, not 256 times.
//   Window: at slot 255 no workgroup starts iteration i + 1 before this
// side's receives of slots 0..254 have landed (kScrLanded, counted by the
// pulling half at its publish points: every nb_publish receives, at slot 254
// and at the last) and its sends of slots 0..254 are drained — a device-scope
// counter of its own (kScrHostSent, counted by the pushing half at its
// publish points), not the grid barrier: a workgroup that is ahead adds and
// goes on, only the flush itself waits.  Slot 255 is waited for by nobody
// before the end.  The end is last_to_finish: every push drained, every pull
// landed and credited.
//   Check mode: the pulling half checksums and poisons its chunk inside
// pull_recv (rx is only ever written by this kernel).  The endpoint receives
// into ONE rx, so push i + 1 is stored only after the endpoint has checked
// and poisoned payload i and said so in its out.credit word (a one-slot
// ring), and every push is published.
//   Workgroup 0 counts the receives the reference's Waitall calls return
// (iters - iters / 256) and digests their checksums, as k_xfer_pull's
// non-blocking end does.  Every wait is bounded (should_stop / give_up).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock, 4) void k_hostlink_duplex(XferArgs a) {
    // statics of 48 bytes: the dynamic region (the staged tx chunk) stays 16-byte aligned
    __shared__ __attribute__((aligned(16))) u64 s_w[6];   // block_sum's four, s_seen, s_abort
    extern __shared__ v4u s_tx[];
    int* s_abort = reinterpret_cast<int*>(&s_w[5]);
    if (threadIdx.x == 0) {
        *s_abort = 0;
        s_w[4] = 0;
    }
    __syncthreads();
    Loop<MPX_MODE_NONBLOCKING, true> L{a, s_abort, s_w, s_tx, {}, &s_w[4]};
    const bool pusher = (int)blockIdx.x < a.nwg;
    L.wg_ = pusher ? (int)blockIdx.x : (int)blockIdx.x - a.nwg;
    const bool reader = L.wg_ == 0;   // this half's reader of host memory
    L.stamp(kTsEntry);
    const long long n = a.len;
    const u64 nw = (u64)a.nwg;
    // Wait until the endpoint's word *host covers `want`.  The half's reader
    // polls it across the link and republishes the value in scratch word
    // `word`; the others poll that.  s_w[4]: the highest value seen so far.
    auto await = [&](const u64* host, int word, u64 want, int iter) -> bool {
        if (threadIdx.x == 0 && s_w[4] < want) {
            const u64 t0 = now_ticks();
            u64 spins = 0;
            for (;;) {
                const u64 v = reader ? ld_sys(host)
                                     : __hip_atomic_load(&a.gbar[word], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (v >= want) {
                    s_w[4] = v;
                    if (reader && a.nwg > 1)
                        __hip_atomic_store(&a.gbar[word], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    break;
                }
                if (L.should_stop(++spins, t0)) { L.give_up(iter); break; }
                __builtin_amdgcn_s_sleep(1);
            }
        }
        __syncthreads();
        return !L.aborted();
    };
    L.post_receives();
    bool ok = true;
    if (pusher && a.iters > 0) {
        // no byte of this call lands in the endpoint's rx before it has entered the call
        if (reader) {
            ok = L.template poll_ge<true>(&a.my_mb->posted[a.peer_slot], a.call, 0);
            if (ok && threadIdx.x == 0 && a.nwg > 1)
                __hip_atomic_store(&a.gbar[kScrHostPosted], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            ok = L.template poll_ge<false>(&a.gbar[kScrHostPosted], 1, 0);
        }
        L.stamp(kTsPosted);
    }
    int inflight = 0;
    u64 pending = 0;   // this workgroup's pushes / pulls since its last publish
    for (int i = 0; ok && i < a.iters; ++i) {
        const int slot = i % kNbWindow;
        const bool last = i + 1 == a.iters;
        const bool pub = (i + 1) % a.nb_publish == 0 || slot == kNbWindow - 2 || last;
        ++pending;
        if (pusher) {                                  // Isend(tx, B)
            // check mode: the endpoint has checked and poisoned payload i - 1
            if (a.check && i > 0 && !await(&a.my_mb->credit[a.peer_slot][0], kScrHostCredit, a.tx_seq0 + (u64)i, i)) {
                ok = false;
                break;
            }
            const bool publish = pub || a.check;
            L.push_bulk(n, a.tx_seq0 + (u64)i + 1, publish, nullptr, a.skip_push == i + 1);
            if (publish) {                             // (drained: push_bulk)
                if (threadIdx.x == 0)
                    __hip_atomic_fetch_add(&a.gbar[kScrHostSent], pending, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                pending = 0;
            }
        } else {                                       // Irecv(rx, B)
            const u64 seq = a.rx_seq0 + (u64)i + 1;
            ok = await(&a.my_mb->ready[a.peer_slot], kScrHostSeen, seq, i) && L.pull_recv(n, seq, i, pub ? pending : 0);
            if (pub) pending = 0;
            if (!ok) break;
        }
        if (inflight == kNbWindow - 1) {
            // Waitall(255, ...): the receives and the sends of slots 0..254
            // (iterations i-255 .. i-1), every workgroup of both halves
            ok = L.template poll_ge<false>(&a.gbar[kScrLanded], nw * (u64)i, i) &&
                 L.template poll_ge<false>(&a.gbar[kScrHostSent], nw * (u64)i, i);
            inflight = 0;
        } else {
            ++inflight;
        }
        if (i == 0) L.stamp(kTsFirst);
    }
    L.stamp(kTsLoop);
    // Waitall(inflight): every workgroup's pushes are drained and its pulls
    // landed and credited once it is here, so the last to finish ends the call
    if (!L.last_to_finish()) return;
    const bool whole = !__hip_atomic_load(&a.gbar[kScrAbort], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    u64 part = 0;
    if (whole && a.check) {
        const u64 fmix = mix64((u64)n);
        for (int j = threadIdx.x; j < a.iters; j += kBlock)
            if (j % kNbWindow != kNbWindow - 1)
                part += __hip_atomic_load(&a.csum[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ^ fmix;
    }
    const u64 s = block_sum(part, s_w);
    if (threadIdx.x == 0) {
        L.rdone = whole ? (u64)(a.iters - a.iters / kNbWindow) : 0;
        L.rdig = s;
        // every other workgroup is done with the relay words and the sent count
        for (int k = kScrHostSeen; k <= kScrHostSent; ++k)
            __hip_atomic_store(&a.gbar[k], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    L.finish_last();
}

// ---------------------------------------------------------------------------
// k_xfer_fan: one rank's side of a fan exchange (mpx_xfer_fan) — a block to
// and from each of several peers in ONE launch.  The grid is the sum of the
// links' widths; workgroup (k, w) (FanTable.map) owns chunk w of link k and
// runs that chunk's whole loop alone: no workgroup waits for another link.
//   * post: workgroup (k, 0) stores this call's number into peer k's mailbox
//     (Mailbox.posted); nothing is pushed to a peer before its post was seen;
//   * push: chunk w of tx block peers[k] into the peer's rx block of this
//     rank — 16-B sc0|sc1 buffer stores (push_units), tx read from HBM/L2
//     (every peer gets another block: no LDS staging) — then, on the
//     non-blocking loop's publish schedule, drain + flag[me][w];
//   * receive: without check mode only the link's last flag of chunk w is
//     waited for; in check mode chunk w of every receive is checksummed and
//     poisoned (all but the last) and credit[me][w] returned to the sender,
//     whose workgroup w pushes iteration i >= 1 only after the credit of
//     i - 1 (else the poison could land on a payload that arrived early);
//   * end of the link: min of the receives completed and max of the end time
//     over the link's workgroups (device atomics into the link's record).
// An empty chunk (lo >= n) moves nothing and still publishes, credits and
// counts.  Every wait is bounded (should_stop / give_up).  The call ends as
// every kernel-engine call does (last_to_finish, finish_last): scratch words
// back to zero, one sealed Fin line.
// ---------------------------------------------------------------------------
// CHECK: check mode's kernel (a call's f.check picks the instantiation, so the
// plain loop carries none of the checking code's registers).  Plain: 48 VGPRs,
// 67 SGPRs; check: 73 VGPRs, 78 SGPRs under amdgpu_num_sgpr(80) — left alone
// the compiler takes 106 SGPRs there, as for every k_xfer kernel; with the
// cap it keeps 38 scalar values in VGPR lanes instead.  No scratch either way
// (DESIGN.md "Fan exchange").
// GEN: where a push's bytes come from (mpx_xfer_fan_seq).  false: the link's tx
// block; true: chunk w of iteration i's pattern under the link's key, generated
// in registers (Loop::gen_units, the tail bytes as push_bulk's SEQ branch) —
// tx is not touched; waits, drain, flag, credit, checksum, poison and both
// ends are the same lines.  The key is derived here from the call's seed, this
// rank and the link's peer, so FanLink and FanTable stay as they are.  Figures
// of the GEN instantiations: DESIGN.md "Sequenced fan payloads".
template <bool CHECK, bool GEN = false>
__global__ __launch_bounds__(kBlock, 4) __attribute__((amdgpu_num_sgpr(80))) void k_xfer_fan(FanArgs f) {
    __shared__ int s_abort;
    __shared__ u64 lds4[4];
    if (threadIdx.x == 0) s_abort = 0;
    XferArgs x{};   // what the shared wait, push and end-of-call helpers read
    x.status = f.status;
    x.gbar = f.gbar;
    x.timeout_ticks = f.timeout_ticks;
    x.done_token = f.done_token;
    x.stream = f.stream;
    x.iters = f.iters;
    Loop<MPX_MODE_NONBLOCKING> L{x, &s_abort, lds4, nullptr, {}};
    __syncthreads();
    L.stamp(kTsEntry);
    const unsigned m = f.tab->map[blockIdx.x];
    const int k = (int)(m >> 16), w = (int)(m & 0xffffu);
    FanLink& lk = f.tab->link[k];
    const long long n = f.len;
    const int nw = lk.nwg;
    const u64 tx0 = lk.tx_seq0, rx0 = lk.rx_seq0;
    // this workgroup's chunk [lo, hi) of the link's block (Loop::chunk_of)
    const long long chunk = (((n + nw - 1) / nw) + 15) & ~15ll;
    const long long lo = (long long)w * chunk;
    const long long hi = lo + chunk < n ? lo + chunk : n;
    const unsigned bytes = lo < hi ? (unsigned)(hi - lo) : 0u;
    const int nv = (int)(bytes >> 4);
    const unsigned tail = bytes & 15;
    const long long at = bytes ? lk.off + lo : 0;       // (an empty chunk touches no memory)
    const unsigned char* src = f.tx + at;
    const __amdgpu_buffer_rsrc_t dst = rsrc(lk.peer_rx + (bytes ? lo : 0), bytes);
    const __amdgpu_buffer_rsrc_t mine = rsrc(f.rx + at, bytes);
    u64* flag_out = &lk.peer_mb->flag[f.my_slot][w];
    u64* credit_out = &lk.peer_mb->credit[f.my_slot][w];
    const u64* flag_in = &f.my_mb->flag[lk.peer][w];
    const u64* credit_in = &f.my_mb->credit[lk.peer][w];
    // GEN: mpx_pattern_key(seed, me, peer, 0), uniform per workgroup; the chunk's first 64-bit word
    u64 key0 = 0, k0 = 0;
    if constexpr (GEN) {
        key0 = f.seq_seed ^ ((u64)(unsigned)f.my_slot << 56) ^ ((u64)(unsigned)lk.peer << 48);
        k0 = (u64)lo >> 3;                              // lo is a multiple of 16
    }

    // bounded one-lane poll of a word a peer writes
    auto wait_ge = [&](const u64* p, u64 want, int iter) -> bool {
        if (threadIdx.x == 0) {
            const u64 t0 = now_ticks();
            u64 spins = 0;
            while (ld_sys(p) < want) {
                if (L.should_stop(++spins, t0)) { L.give_up(iter); break; }
                __builtin_amdgcn_s_sleep(1);
            }
        }
        __syncthreads();
        return !L.aborted();
    };

    if (w == 0 && threadIdx.x == 0) st_sys(&lk.peer_mb->posted[f.my_slot], lk.call);
    bool ok = f.iters == 0 || wait_ge(&f.my_mb->posted[lk.peer], lk.call, 0);
    L.stamp(kTsPosted);
    u64 done = 0;
    for (int i = 0; ok && i < f.iters; ++i) {
        if (CHECK && i > 0) {                        // chunk w of push i - 1 was checked: its poison is in
            ok = wait_ge(credit_in, tx0 + (u64)i, i);
            if (!ok) break;
        }
        if (bytes && f.skip_push != i + 1) {           // (test knob: this payload is "lost")
            if constexpr (GEN) {
                const u64 key = key0 ^ ((u64)(unsigned)i << 24);
                if (f.stream) L.template gen_units<kAuxSysNt>(dst, nv, key, k0);
                else L.template gen_units<kAuxSys>(dst, nv, key, k0);
                if (threadIdx.x < tail) {                  // the one or two words the tail bytes fall in
                    const unsigned o = (unsigned)nv * 16 + threadIdx.x;
                    const u64 wd = fill_word(key, k0 + (o >> 3));
                    __builtin_amdgcn_raw_buffer_store_b8((unsigned char)(wd >> (8 * (o & 7))), dst, o, 0, kAuxSys);
                }
            } else {
                L.push_units_aux<false>(reinterpret_cast<const v4u*>(src), dst, nv);
                if (threadIdx.x < tail) {
                    const unsigned o = (unsigned)nv * 16 + threadIdx.x;
                    __builtin_amdgcn_raw_buffer_store_b8(src[o], dst, o, 0, kAuxSys);
                }
            }
        }
        if (CHECK || (i + 1) % f.nb_publish == 0 || i + 1 == f.iters) {
            drain_stores();                            // every storing wave
            __syncthreads();
            if (threadIdx.x == 0) st_sys(flag_out, tx0 + (u64)i + 1);
        }
        if constexpr (CHECK) {
        ok = wait_ge(flag_in, rx0 + (u64)i + 1, i);
        if (!ok) break;
        // checksum (word indices count from the block's start) and poison
        // this chunk of receive i, as Loop::sum_chunk does for a pair's
        const bool keep = i + 1 == f.iters;
        const u64 poison = 0x5a5a5a5a5a5a5a5aull ^ (u64)i;
        u64 acc = 0;
        if (threadIdx.x == 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
        drain_stores();
        __syncthreads();
        if (bytes) {
            const v4u pv = {(unsigned)poison, (unsigned)(poison >> 32), (unsigned)poison, (unsigned)(poison >> 32)};
            for (int v = threadIdx.x; v < nv; v += kBlock) {
                const v4u q = __builtin_amdgcn_raw_buffer_load_b128(mine, v * 16, 0, kAuxSys);
                const u64 kw = (u64)(lo / 8) + 2 * (u64)v;
                acc += csum_term(((u64)q.y << 32) | q.x, kw);
                acc += csum_term(((u64)q.w << 32) | q.z, kw + 1);
                if (!keep) __builtin_amdgcn_raw_buffer_store_b128(pv, mine, v * 16, 0, kAuxSys);
            }
            if (threadIdx.x < 2 && 8 * threadIdx.x < tail) {   // only the block's last chunk has a tail
                const unsigned o = (unsigned)nv * 16 + 8 * threadIdx.x;
                u64 word = 0;
                for (unsigned b = 0; b < 8 && o + b < bytes; ++b)
                    word |= (u64)__builtin_amdgcn_raw_buffer_load_b8(mine, o + b, 0, kAuxSys) << (8 * b);
                acc += csum_term(word, (u64)(lo + o) / 8);
            }
            __syncthreads();
            if (!keep && threadIdx.x < tail)
                __builtin_amdgcn_raw_buffer_store_b8((unsigned char)poison, mine, (unsigned)nv * 16 + threadIdx.x, 0,
                                                     kAuxSys);
        }
        drain_stores();                                // the poison is in before the credit goes
        const u64 s = block_sum(acc, lds4);
        if (threadIdx.x == 0) {
            if (s) atomicAdd(&f.csum[lk.csum0 + i], s);
            st_sys(credit_out, rx0 + (u64)i + 1);
        }
        ++done;
        }
    }
    L.stamp(kTsLoop);
    // Waitall: without check mode, the link's last flag of this chunk
    if (!CHECK && ok && f.iters > 0 && wait_ge(flag_in, rx0 + (u64)f.iters, f.iters - 1)) done = (u64)f.iters;
    drain_stores();
    __syncthreads();
    if (threadIdx.x == 0) {
        __hip_atomic_fetch_min(&lk.recv_done, done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(&lk.t_end, now_ticks(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (!L.last_to_finish()) return;
    // workgroup 0, every other workgroup done: the call's receive count and
    // digest (of a call that completed: a timeout fails it anyway)
    u64 part = 0, dpart = 0;
    for (int j = threadIdx.x; j < f.nlinks; j += kBlock)
        part += __hip_atomic_load(&f.tab->link[j].recv_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (CHECK && !__hip_atomic_load(&f.gbar[kScrAbort], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
        const u64 fmix = mix64((u64)n);
        for (int j = threadIdx.x; j < f.nlinks * f.iters; j += kBlock)
            dpart += __hip_atomic_load(&f.csum[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ^ fmix;
    }
    const u64 d = block_sum(part, lds4);
    const u64 g = block_sum(dpart, lds4);
    if (threadIdx.x == 0) {
        L.rdone = d;
        L.rdig = g;
    }
    L.finish_last();
}

// ---------------------------------------------------------------------------
// k_xfer_fan_ll: the fan exchange with MPX_FAN_LL — per link a LOCK-STEP
// exchange of LL granules (MPI_Sendrecv with every peer, per iteration).  The
// grid is nlinks: workgroup k IS link k (no workgroup map) and runs the link's
// whole loop alone, so no iteration of one link waits for another link.
//   * post: the workgroup's first action is this call's number into the
//     peer's Mailbox.posted; nothing is pushed before the peer's post is seen
//     (once per call, as in k_xfer_fan);
//   * preload: the link's tx block is read ONCE into VGPRs (Loop::preload_ll;
//     <= 4096 B = 512 units, two per lane), so every push is stores only;
//   * iteration i: push number s = tx_seq0 + i + 1 as LL units {lo, tag, hi,
//     tag} into half s & 1 of the peer's ll[me] row (16-B sc0|sc1 buffer
//     stores, no drain, no flag); poll half r & 1 of my ll[peer] row for the
//     peer's push r = rx_seq0 + i + 1 (all of a lane's 16-B volatile loads
//     back to back, both tags of each checked); unpack into the link's rx
//     block with write-through stores; check mode then reads the block back
//     (sc0 sc1), checksums it into csum[k * iters + i] and poisons all but
//     the last (Loop::check's LL branch: the poison lands in my own rx, the
//     peer writes only my LL row, so no credit).
// Two halves suffice without credits: I push i + 1 only after I received the
// peer's i; the peer pushed its i before it started to wait for my i, so it
// may still be polling my i — which sits in the other half.  My i + 2 reuses
// the half of my i and goes out only after I received the peer's i + 1, which
// the peer issued only after its poll of my i had the data in registers
// (DESIGN.md "Fan exchange").
// Test knobs: skip_push = i — push i's tags arrive with a wrong payload;
// lag — this link's workgroup stalls between its push and its wait of
// iteration iters / 2, where a single-buffered zone would break.
// Every wait is bounded (should_stop / give_up); the call ends as k_xfer_fan's
// does.  Resource figures: DESIGN.md "Fan exchange".
// LAT is the traced form (mpx_fan_lat_*; LatTrace<true, true>): lane 0 of
// EVERY workgroup is a tracer, into the block of its link's peer (q.lat + peer
// * q.lat_stride).  t[0] is a clock read of the link's own behind the posted
// wait (Loop::stamp records workgroup 0 only, for the Fin line); t[i + 1] is
// read at the bottom of iteration i, behind wait_ll and the check.  The fold
// (end) comes before the workgroup counts itself out.
// One kernel template, the traced lines under `if constexpr (LAT)`: a template
// parameter on the kernel itself costs nothing — the LAT = false instantiations
// are instruction for instruction the kernels that had no recorder, the LAT =
// true ones the traced copy this replaced.  A `__device__` body shared between
// kernels is NOT free: routing this loop, or the end-of-call code below, through
// one changes the callers' register allocation (k_xfer_fan: 73 -> 75 VGPRs),
// so the body stands here in the kernel, and k_xfer_fan keeps end-of-call code
// of its own (DESIGN.md "Link recorder").
// GEN (mpx_xfer_fan_seq): no preload; iteration i's units are generated from
// the link's key (Loop::gen_ll) before every push_ll.  A skipped push stays
// push_ll_tags_only.  Never traced: there is no LAT && GEN instantiation.
// ---------------------------------------------------------------------------
template <bool CHECK, bool LAT, bool GEN = false>
__global__ __launch_bounds__(kBlock, 4) __attribute__((amdgpu_num_sgpr(80))) void k_xfer_fan_ll(FanLLArgs q) {
    static_assert(!(LAT && GEN), "a sequenced LL fan call is never traced");
    __shared__ int s_abort;
    __shared__ u64 lds4[4];
    if (threadIdx.x == 0) s_abort = 0;
    const FanArgs& f = q.f;
    const int k = (int)blockIdx.x;
    FanLink& lk = f.tab->link[k];
    const long long n = f.len;
    XferArgs x{};   // the link as a pair: what Loop's LL, wait and end-of-call helpers read
    x.tx = f.tx + lk.off;
    x.rx = f.rx + lk.off;
    x.my_mb = f.my_mb;
    x.peer_mb = lk.peer_mb;
    x.my_slot = f.my_slot;
    x.peer_slot = lk.peer;
    x.status = f.status;
    x.gbar = f.gbar;
    x.csum = f.csum + lk.csum0;
    x.timeout_ticks = f.timeout_ticks;
    x.done_token = f.done_token;
    x.iters = f.iters;
    x.ll_max = MPX_FAN_LL_MAX;
    Loop<MPX_MODE_PINGPONG, true, GEN> L{x, &s_abort, lds4, nullptr, {}};
    __syncthreads();
    L.stamp(kTsEntry);
    const u64 tx0 = lk.tx_seq0, rx0 = lk.rx_seq0;
    if (threadIdx.x == 0) st_sys(&lk.peer_mb->posted[f.my_slot], lk.call);
    u64 key0 = 0;   // GEN: mpx_pattern_key(seed, me, peer, 0)
    if constexpr (GEN) key0 = f.seq_seed ^ ((u64)(unsigned)f.my_slot << 56) ^ ((u64)(unsigned)lk.peer << 48);
    else L.preload_ll(n);
    bool ok = f.iters > 0;
    if (ok) {
        if (threadIdx.x == 0) {
            const u64 t0 = now_ticks();
            u64 spins = 0;
            while (ld_sys(&f.my_mb->posted[lk.peer]) < lk.call) {
                if (L.should_stop(++spins, t0)) { L.give_up(0); break; }
                __builtin_amdgcn_s_sleep(1);
            }
        }
        __syncthreads();
        ok = !L.aborted();
    }
    L.stamp(kTsPosted);
    LatTrace<LAT, true> T;
    if constexpr (LAT) {
        if (T.on()) {   // t[0]: this link's own read, behind its own posted wait
            const u64 t = lat_stamp();
            T.begin(reinterpret_cast<LatBlock*>(q.lat + (u64)lk.peer * q.lat_stride), t, t, f.iters);
        }
    }
    u64 done = 0;
    for (int i = 0; ok && i < f.iters; ++i) {
        const u64 s = tx0 + (u64)i + 1, r = rx0 + (u64)i + 1;
        const unsigned out = (unsigned)(s & 1) * kFanLLHalf, in = (unsigned)(r & 1) * kFanLLHalf;
        if (f.skip_push == i + 1) {
            L.push_ll_tags_only(n, s, out);                        // (test knob: this payload is "lost")
        } else {
            if constexpr (GEN) L.gen_ll(n, key0 ^ ((u64)(unsigned)i << 24));
            L.push_ll(n, s, out);
        }
        if (q.lag_ticks && k == q.lag_link && i == f.iters / 2) {   // (test knob)
            if (threadIdx.x == 0) {
                const u64 t0 = now_ticks();
                while (now_ticks() - t0 < q.lag_ticks) __builtin_amdgcn_s_sleep(127);
            }
            __syncthreads();
        }
        ok = L.wait_ll(n, r, i, in);
        if (!ok) break;
        ++done;
        if constexpr (CHECK) L.check(n, i);
        if constexpr (LAT) {
            if (T.on()) T.tick(i);   // one clock read: the bottom of iteration i
        }
    }
    L.stamp(kTsLoop);
    if constexpr (LAT) T.end();   // (before the drain: the fold's stores are out when the workgroup counts itself out)
    // the end of the link and of the call, as in k_xfer_fan
    drain_stores();
    __syncthreads();
    if (threadIdx.x == 0) {
        __hip_atomic_fetch_min(&lk.recv_done, done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(&lk.t_end, now_ticks(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (!L.last_to_finish()) return;
    // workgroup 0, every other workgroup done: the call's receive count and
    // digest (of a call that completed: a timeout fails it anyway)
    u64 part = 0, dpart = 0;
    for (int j = threadIdx.x; j < f.nlinks; j += kBlock)
        part += __hip_atomic_load(&f.tab->link[j].recv_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (CHECK && !__hip_atomic_load(&f.gbar[kScrAbort], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
        const u64 fmix = mix64((u64)n);
        for (int j = threadIdx.x; j < f.nlinks * f.iters; j += kBlock)
            dpart += __hip_atomic_load(&f.csum[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ^ fmix;
    }
    const u64 d = block_sum(part, lds4);
    const u64 g = block_sum(dpart, lds4);
    if (threadIdx.x == 0) {
        L.rdone = d;
        L.rdig = g;
    }
    L.finish_last();
}

// stream engines' receive accounting (launch_account)
__global__ __launch_bounds__(kBlock) void k_account(Status* st, const u64* csum, int j0, int count, u64 fmix) {
    __shared__ u64 lds4[4];
    u64 part = 0;
    if (csum)
        for (int j = threadIdx.x; j < count; j += kBlock) part += csum[j0 + j] ^ fmix;
    const u64 s = block_sum(part, lds4);
    if (threadIdx.x == 0) {
        const u64 d = __hip_atomic_load(&st->recv_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        const u64 g = __hip_atomic_load(&st->recv_digest, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&st->recv_done, d + (u64)count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&st->recv_digest, g + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
hipError_t launch_xfer(const XferArgs& a, int grid, hipStream_t s) {
    (void)hipGetLastError();   // drop a stale error of an earlier, ignored call
    void (*k)(XferArgs) = nullptr;
    // a sequenced call (mpx_xfer_seq): never traced, never pulled, no LDS stage
    if (a.seq) {
        if (a.lat || a.pull || a.stage) return hipErrorInvalidValue;
        switch (a.mode) {
            case MPX_MODE_PINGPONG: k = a.group ? k_xfer_seq<MPX_MODE_PINGPONG, 1> : k_xfer_seq<MPX_MODE_PINGPONG, 0>; break;
            case MPX_MODE_UNIDIR: k = a.group ? k_xfer_seq<MPX_MODE_UNIDIR, 1> : k_xfer_seq<MPX_MODE_UNIDIR, 0>; break;
            case MPX_MODE_NONBLOCKING:   // both sides alike
                k = a.check ? k_xfer_seq_nbcheck : k_xfer_seq<MPX_MODE_NONBLOCKING, 0>;
                break;
            default: return hipErrorInvalidValue;
        }
        hipLaunchKernelGGL(k, dim3(grid), dim3(kBlock), 0, s, a);
        return hipGetLastError();
    }
    // tracing on (a.lat): the blocking loops' traced instantiations; the
    // non-blocking loop has none and must not be handed a recorder
    if (a.lat) {
        if (a.mode != MPX_MODE_PINGPONG && a.mode != MPX_MODE_UNIDIR) return hipErrorInvalidValue;
        const bool pp = a.mode == MPX_MODE_PINGPONG;
        if (a.pull)
            k = pp ? (a.group ? k_xfer_pull_lat<MPX_MODE_PINGPONG, 1> : k_xfer_pull_lat<MPX_MODE_PINGPONG, 0>)
                   : (a.group ? k_xfer_pull_lat<MPX_MODE_UNIDIR, 1> : k_xfer_pull_lat<MPX_MODE_UNIDIR, 0>);
        else
            k = pp ? (a.group ? k_xfer_lat<MPX_MODE_PINGPONG, 1> : k_xfer_lat<MPX_MODE_PINGPONG, 0>)
                   : (a.group ? k_xfer_lat<MPX_MODE_UNIDIR, 1> : k_xfer_lat<MPX_MODE_UNIDIR, 0>);
        hipLaunchKernelGGL(k, dim3(grid), dim3(kBlock), a.pull ? 0u : (unsigned)a.stage, s, a);
        return hipGetLastError();
    }
    if (a.pull) {
        switch (a.mode) {
            case MPX_MODE_PINGPONG: k = a.group ? k_xfer_pull<MPX_MODE_PINGPONG, 1> : k_xfer_pull<MPX_MODE_PINGPONG, 0>; break;
            case MPX_MODE_UNIDIR: k = a.group ? k_xfer_pull<MPX_MODE_UNIDIR, 1> : k_xfer_pull<MPX_MODE_UNIDIR, 0>; break;
            case MPX_MODE_NONBLOCKING: k = k_xfer_pull<MPX_MODE_NONBLOCKING, 0>; break;   // both sides alike
            default: return hipErrorInvalidValue;
        }
        hipLaunchKernelGGL(k, dim3(grid), dim3(kBlock), 0, s, a);
        return hipGetLastError();
    }
    switch (a.mode) {
        case MPX_MODE_PINGPONG: k = a.group ? k_xfer<MPX_MODE_PINGPONG, 1> : k_xfer<MPX_MODE_PINGPONG, 0>; break;
        case MPX_MODE_UNIDIR: k = a.group ? k_xfer<MPX_MODE_UNIDIR, 1> : k_xfer<MPX_MODE_UNIDIR, 0>; break;
        case MPX_MODE_NONBLOCKING:   // both sides alike
            k = a.check ? k_xfer_nbcheck : k_xfer<MPX_MODE_NONBLOCKING, 0>;
            break;
        default: return hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(k, dim3(grid), dim3(kBlock), (unsigned)a.stage, s, a);
    return hipGetLastError();
}

hipError_t launch_hostlink(const XferArgs& a, int grid, hipStream_t s) {
    // the kernel indexes flag / credit words by workgroup and LL granules by length
    if (grid < 1 || grid > kMaxPushWG || a.nwg < 1 || a.nwg > kMaxPushWG || (grid != 1 && grid != a.nwg) ||
        a.ll_max < 0 || a.ll_max > kLLMaxBytes || a.len < 0 || a.stage < 0 || a.stage > kStageMaxBytes)
        return hipErrorInvalidValue;
    (void)hipGetLastError();   // drop a stale error of an earlier, ignored call
    void (*k)(XferArgs) = nullptr;
    // a sequenced call (mpx_xfer_hostlink_seq): never traced, no LDS stage
    if (a.seq) {
        if (a.lat || a.stage) return hipErrorInvalidValue;
        switch (a.mode) {
            case MPX_MODE_PINGPONG: k = a.group ? k_hostlink_gen<MPX_MODE_PINGPONG, 1> : k_hostlink_gen<MPX_MODE_PINGPONG, 0>; break;
            case MPX_MODE_UNIDIR: k = a.group ? k_hostlink_gen<MPX_MODE_UNIDIR, 1> : k_hostlink_gen<MPX_MODE_UNIDIR, 0>; break;
            default: return hipErrorInvalidValue;
        }
        hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(kBlock), 0, s, a);
        return hipGetLastError();
    }
    switch (a.mode) {
        case MPX_MODE_PINGPONG:
            // the host-link recorder on (a.lat): the traced instantiations
            if (a.lat) k = a.group ? k_hostlink_lat<MPX_MODE_PINGPONG, 1> : k_hostlink_lat<MPX_MODE_PINGPONG, 0>;
            else k = a.group ? k_xfer_hostlink<MPX_MODE_PINGPONG, 1> : k_xfer_hostlink<MPX_MODE_PINGPONG, 0>;
            break;
        case MPX_MODE_UNIDIR:
            if (a.lat) k = a.group ? k_hostlink_lat<MPX_MODE_UNIDIR, 1> : k_hostlink_lat<MPX_MODE_UNIDIR, 0>;
            else k = a.group ? k_xfer_hostlink<MPX_MODE_UNIDIR, 1> : k_xfer_hostlink<MPX_MODE_UNIDIR, 0>;
            break;
        default: return hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(kBlock), (unsigned)a.stage, s, a);
    return hipGetLastError();
}

hipError_t launch_hostlink_duplex(const XferArgs& a, hipStream_t s) {
    // the kernel indexes flag / credit words by workgroup, and its window arithmetic divides by nb_publish
    if (a.nwg < 1 || a.nwg > kDuplexMaxWG || a.len < 0 || a.iters < 0 || a.stage < 0 || a.stage > kStageMaxBytes ||
        a.nb_publish < 1 || kNbWindow % a.nb_publish != 0)
        return hipErrorInvalidValue;
    (void)hipGetLastError();   // drop a stale error of an earlier, ignored call
    hipLaunchKernelGGL(k_hostlink_duplex, dim3(2u * (unsigned)a.nwg), dim3(kBlock), (unsigned)a.stage, s, a);
    return hipGetLastError();
}

hipError_t launch_fan(const FanArgs& a, int grid, hipStream_t s) {
    if (grid < 1 || grid > kFanMaxGrid) return hipErrorInvalidValue;
    (void)hipGetLastError();   // drop a stale error of an earlier, ignored call
    // a sequenced call (mpx_xfer_fan_seq): the generating instantiations
    void (*k)(FanArgs) = a.seq ? (a.check ? k_xfer_fan<true, true> : k_xfer_fan<false, true>)
                               : (a.check ? k_xfer_fan<true> : k_xfer_fan<false>);
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_fan_ll(const FanLLArgs& a, hipStream_t s) {
    if (a.f.nlinks < 1 || a.f.nlinks >= MPX_MAX_RANKS || a.f.len < 0 || a.f.len > MPX_FAN_LL_MAX) return hipErrorInvalidValue;
    (void)hipGetLastError();   // drop a stale error of an earlier, ignored call
    // the link recorder on (a.lat): the traced instantiations
    if (a.lat && a.lat_stride < sizeof(LatBlock)) return hipErrorInvalidValue;
    void (*k)(FanLLArgs) = a.lat ? (a.f.check ? k_xfer_fan_ll<true, true> : k_xfer_fan_ll<false, true>)
                                 : (a.f.check ? k_xfer_fan_ll<true, false> : k_xfer_fan_ll<false, false>);
    // a sequenced call (mpx_xfer_fan_seq) is never traced: it has no traced instantiation
    if (a.f.seq) {
        if (a.lat) return hipErrorInvalidValue;
        k = a.f.check ? k_xfer_fan_ll<true, false, true> : k_xfer_fan_ll<false, false, true>;
    }
    hipLaunchKernelGGL(k, dim3((unsigned)a.f.nlinks), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}

// One k_copy form, from the tuning sweeps (DESIGN.md "k_copy tuning"): ONE
// 16-B unit per lane and ONE step per block — grid = n/4 KiB workgroups of
// 256 lanes, no cap, nontemporal loads and stores.  6.51-6.53 TB/s of HBM
// traffic at 256 MiB, 1 GiB and 4 GiB alike (profiles/r01_copy_lab_onestep.jsonl),
// against 6.0 / 5.45 TB/s for the earlier contiguous-chunk form and 4.76 TB/s
// for hipMemcpyAsync device-to-device.  The 39 other instantiations of round
// 1-3's variant knob (unroll x load/store policy x layout) are gone; their
// evidence stays in profiles/copy_sweep_r01.jsonl and r01_copy_policy_*.
// win.on: k_copy_win, the same form with a striped part of src loaded with
// the default policy (the rule and its evidence at copy_window_rule).
hipError_t launch_copy(void* dst, const void* src, size_t n, hipStream_t s, int* grid_out, const CopyWindow& win) {
    const size_t n16 = n / 16;
    const unsigned tail = (unsigned)(n & 15);
    size_t grid = (n16 + (size_t)kBlock - 1) / (size_t)kBlock;
    if (grid < 1) grid = 1;
    if (grid > ((size_t)1 << 31) - 1) return hipErrorInvalidValue;
    if (grid_out) *grid_out = (int)grid;
    (void)hipGetLastError();   // drop a stale error of an earlier, ignored call
    if (win.on) {
        // n16 == 0 (n < 16): one workgroup, nothing kept, only the tail bytes
        hipLaunchKernelGGL(k_copy_win, dim3((unsigned)grid), dim3(kBlock), 0, s, reinterpret_cast<const v4u*>(src),
                           reinterpret_cast<v4u*>(dst), n16, tail, (unsigned)__builtin_ctz(win.unit), win.period - 1,
                           n16 ? win.window : 0u);
        return hipGetLastError();
    }
    hipLaunchKernelGGL((k_copy<1, true, true, false>), dim3((unsigned)grid), dim3(kBlock), 0, s,
                       reinterpret_cast<const v4u*>(src), reinterpret_cast<v4u*>(dst), n16, tail);
    return hipGetLastError();
}

hipError_t launch_copy_steps(void* dst, const void* src, size_t n, int iters, u64* bar, hipStream_t s,
                             int* grid_out, const int* shape) {
    // Defaults from the A/Bs: at most 64 workgroups and one hot counter
    // (fewer arrivals beat more lanes: 1 MiB 2.08 us vs 2.40 with 256,
    // profiles/r02_copy_steps_variants.jsonl); no store drain before arrival
    // (the barrier orders issue, not acknowledgement: -0.05..0.1 us per step).
    // Workgroups of 1024 lanes, one unit per lane: 16 KiB per workgroup per
    // step, so up to 16 KiB a copy is ONE workgroup and its steps need no
    // grid barrier (__syncthreads ends a step), and up to 1 MiB at most 64
    // workgroups arrive at the barrier.  Against the 256-lane grid sized for
    // 1-8 units per lane: 8 KiB 0.96 -> 0.62 us per copy, 16 KiB 0.99 ->
    // 0.70, 32-64 KiB 1.29-1.34 -> 1.12-1.15, 256-512 KiB 1.71-1.86 ->
    // 1.48-1.67, 128 KiB and 1 MiB unchanged; one wide workgroup with more
    // units per lane loses from 32 KiB (one CU's bandwidth)
    // (profiles/r02_copy_steps_wgsize.jsonl).  Above 1 MiB (only when
    // MPX_COPY_STEPS_MAX raises the switch) the 64 workgroups are 256 lanes
    // with 8 units per lane, all loads of a step in flight at once: 2 MiB
    // 2.35 us against 2.56-3.07 with 1024 lanes x 2
    // (r02_copy_steps_wgsize_mid.jsonl, r02_copy_sweep_state.jsonl).
    // `shape` (tests only: MPX_COPY="steps:..." via mpx_copy) overrides
    // {grid_cap, xcd, drain, upl, threads, one_xcd}.
    // Default-policy loads instead of nontemporal ones change nothing here,
    // fresh or after 1 GiB copies evicted src (r02_copy_steps_ldpolicy.jsonl,
    // measured with a knob since removed).
    // One XCD: from 32 KiB to 512 KiB every working workgroup sits on XCD 0
    // (8x the grid, the others exit at once), so the barrier's arrivals stay
    // within one XCD: 32-64 KiB 1.16-1.20 -> 1.02 us per copy (512 lanes),
    // 128 KiB 1.42 -> 1.12, 256 KiB 1.49 -> 1.25, 512 KiB 1.66 -> 1.53
    // (1024 lanes); at 1 MiB XCD 0's 32 CUs are too few (2.12 vs 1.98)
    // (profiles/r02_copy_steps_onexcd.jsonl).
    int cap = 64, xcd = 0, drain = 0, threads = 1024, upl = 1, one_xcd = 0;
    if (n > ((size_t)16 << 10) && n <= ((size_t)512 << 10)) {
        one_xcd = 1;
        threads = n <= ((size_t)128 << 10) ? 512 : 1024;
    } else if (n > ((size_t)1 << 20)) {
        threads = kBlock;
        upl = 8;
    }
    if (shape) {
        cap = shape[0]; xcd = shape[1]; drain = shape[2]; upl = shape[3]; threads = shape[4]; one_xcd = shape[5];
    }
    if (threads != 512 && threads != 1024) threads = kBlock;
    // the grid barrier needs every workgroup resident: at most the waves of
    // kCopyStepsMaxGrid 256-lane workgroups (4 per CU), whatever the width
    int max_grid = kCopyStepsMaxGrid * kBlock / threads;
    if (one_xcd) {           // the working workgroups share XCD 0's 32 CUs
        max_grid /= 8;
        xcd = 0;
    }
    if (cap < 1 || cap > max_grid) cap = max_grid;
    if (upl < 1) upl = 1;
    const size_t n16 = n / 16;
    size_t grid = (n16 + (size_t)threads * upl - 1) / ((size_t)threads * upl);
    if (grid > (size_t)cap) grid = (size_t)cap;
    if (grid < 1) grid = 1;
    if (grid_out) *grid_out = (int)grid;
    (void)hipGetLastError();   // drop a stale error of an earlier, ignored call
    void (*k)(const v4u*, v4u*, size_t, unsigned, int, u64*, int, int) =
        threads == 1024 ? (xcd ? k_copy_steps<1024, true> : k_copy_steps<1024, false>)
        : threads == 512 ? (xcd ? k_copy_steps<512, true> : k_copy_steps<512, false>)
                         : (xcd ? k_copy_steps<kBlock, true> : k_copy_steps<kBlock, false>);
    hipLaunchKernelGGL(k, dim3((unsigned)(one_xcd ? grid * 8 : grid)), dim3((unsigned)threads), 0, s,
                       reinterpret_cast<const v4u*>(src), reinterpret_cast<v4u*>(dst), n16, (unsigned)(n & 15), iters,
                       bar, drain, one_xcd);
    return hipGetLastError();
}

// All `iters` copies in one k_copy_pipe launch: UPL units per lane chosen so
// the grid (<= kCopyPipeMaxGrid workgroups of 320 lanes, all resident) covers
// n; returns hipErrorInvalidValue when n is too large for a resident grid.
hipError_t launch_copy_pipe(void* dst, const void* src, size_t n, int iters, u64* bar, hipStream_t s,
                            int* grid_out, int upl_force, int hier_force) {
    const size_t n16 = n / 16;
    const size_t lanes = (size_t)kPipeCopyWaves * 64;
    // resident grid: 5-wave workgroups, as many per CU as the VGPRs allow
    // (UPL 16: 208 VGPRs, one per CU; UPL 8: 112, three; UPL <= 4: six)
    auto cap_of = [](int u) -> size_t { return u >= 16 ? 256 : u >= 8 ? 512 : (size_t)kCopyPipeMaxGrid; };
    // Shape.  Up to 1 MiB: 8 units per lane and one barrier counter — few
    // wide workgroups (16-32), because one counter's cost grows with its
    // arrivals (at 2 MiB: 64 workgroups 2.11 us per copy, 256 4.04, 512 7.8;
    // r03_copy_pipe_ab.jsonl).  Above: the two-level barrier (8 group
    // counters in parallel, per-group release words) with up to 256
    // workgroups of 4-16 units per lane: 4 MiB 2.56-2.59 us, 8 MiB 3.2-3.9,
    // 16 MiB 4.3-6.0 against 2.9-3.0 / 3.2-4.2 / 5.0-6.8 for a launch per
    // copy.  The one-counter form with 64+ workgroups read 3.07-3.14 at 2 MiB
    // in three of four bench.py sweeps (2.08-2.14 in a fresh process), and
    // 4.3-6.2 at 4-8 MiB after 1 GiB copies (r03_copy_pipe_hier.jsonl,
    // r03_copy_pipe_state.jsonl).
    const bool big = n > ((size_t)1 << 20);
    int upl = big ? 4 : 8;
    while (big && upl < 16 && (n16 + lanes * upl - 1) / (lanes * upl) > 256) upl *= 2;
    if (upl_force > 0) upl = upl_force;   // tests: every units-per-lane form
    upl = upl <= 1 ? 1 : upl <= 2 ? 2 : upl <= 4 ? 4 : upl <= 8 ? 8 : 16;
    size_t grid = (n16 + lanes * upl - 1) / (lanes * upl);
    while (grid > cap_of(upl) && upl < 16) {
        upl *= 2;
        grid = (n16 + lanes * upl - 1) / (lanes * upl);
    }
    if (grid > cap_of(upl) || n >= ((size_t)1 << 32)) return hipErrorInvalidValue;
    if (grid < 1) grid = 1;
    if (grid_out) *grid_out = (int)grid;
    // (nontemporal loads: default-policy ones read the same, fresh or after
    // 1 GiB copies, 2-8 MiB within 0.03 us: profiles/r03_copy_pipe_state.jsonl)
    void (*k)(const v4u*, v4u*, size_t, unsigned, int, u64*, int) =
        upl <= 1 ? k_copy_pipe<1> : upl <= 2 ? k_copy_pipe<2> : upl <= 4 ? k_copy_pipe<4>
        : upl <= 8 ? k_copy_pipe<8> : k_copy_pipe<16>;
    const int hier = hier_force >= 0 ? (hier_force != 0) : (big ? 1 : 0);   // tests: both barrier forms
    (void)hipGetLastError();   // drop a stale error of an earlier, ignored call
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(kPipeThreads), 0, s, reinterpret_cast<const v4u*>(src),
                       reinterpret_cast<v4u*>(dst), n16, (unsigned)(n & 15), iters, bar, hier);
    return hipGetLastError();
}

hipError_t launch_fill(void* p, size_t n, int pattern, u64 arg, hipStream_t s) {
    size_t grid = (n / 8 + kBlock - 1) / kBlock;
    if (grid > 4096) grid = 4096;
    if (grid < 1) grid = 1;
    (void)hipGetLastError();   // drop a stale error of an earlier, ignored call
    hipLaunchKernelGGL(k_fill, dim3((unsigned)grid), dim3(kBlock), 0, s, reinterpret_cast<unsigned char*>(p), n,
                       pattern, arg);
    return hipGetLastError();
}

hipError_t launch_checksum(const void* p, size_t n, u64* out_dev, hipStream_t s) {
    size_t grid = (n / 16 + kBlock - 1) / kBlock;
    if (grid > 2048) grid = 2048;
    if (grid < 1) grid = 1;
    (void)hipGetLastError();   // drop a stale error of an earlier, ignored call
    hipLaunchKernelGGL(k_checksum, dim3((unsigned)grid), dim3(kBlock), 0, s, reinterpret_cast<const unsigned char*>(p),
                       n, out_dev);
    return hipGetLastError();
}

hipError_t launch_signal(u64* flag, const u64* base, u64 value, hipStream_t s) {
    (void)hipGetLastError();   // drop a stale error of an earlier, ignored call
    hipLaunchKernelGGL(k_signal, dim3(1), dim3(64), 0, s, flag, base, value);
    return hipGetLastError();
}

hipError_t launch_wait(const u64* flag, const u64* base, u64 value, Status* st, u64 timeout_ticks, hipStream_t s) {
    (void)hipGetLastError();   // drop a stale error of an earlier, ignored call
    hipLaunchKernelGGL(k_wait, dim3(1), dim3(64), 0, s, flag, base, value, st, timeout_ticks);
    return hipGetLastError();
}

hipError_t launch_seqbase(u64* base, u64 tx, u64 rx, int add, hipStream_t s) {
    (void)hipGetLastError();   // drop a stale error of an earlier, ignored call
    hipLaunchKernelGGL(k_seqbase, dim3(1), dim3(64), 0, s, base, tx, rx, add);
    return hipGetLastError();
}

hipError_t launch_account(Status* st, const u64* csum, int j0, int count, long long n, hipStream_t s) {
    const u64 z = (u64)n;
    u64 m = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;   // mix64(n), host side
    m = (m ^ (m >> 27)) * 0x94d049bb133111ebull;
    m ^= m >> 31;
    (void)hipGetLastError();   // drop a stale error of an earlier, ignored call
    hipLaunchKernelGGL(k_account, dim3(1), dim3(kBlock), 0, s, st, csum, j0, count, m);
    return hipGetLastError();
}

}  // namespace mpx
