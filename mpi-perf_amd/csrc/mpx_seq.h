// mpx_seq.h — the host side of the sequenced payloads (include/mpx_seq.h):
// the pattern a sequenced call's pushing kernel generates, byte for byte, and
// the checksum its receiver must find.  Plain C++: no HIP include, so the
// file builds with g++ alone (tools/seq_host_check.cpp runs it under the host
// sanitizers).
//
// P(seed, s, d, i, n) is the first n bytes mpx_fill(MPX_FILL_SPLITMIX,
// mpx_pattern_key(seed, s, d, i)) writes: 64-bit word k = fill_word(key, k),
// tail bytes little-endian from the same word (k_fill, mpx_kernels.hip).
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/mpx.h"

namespace mpx {
namespace seq {

constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;

inline uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
// MPX_FILL_SPLITMIX word k
inline uint64_t fill_word(uint64_t key, uint64_t k) { return mix64((key ^ k) + kGolden); }

// the key of the message rank src sends to rank dst in iteration iter: `base`
// is the link's (iteration 0's), which the kernels get in XferArgs
inline uint64_t key_base(uint64_t seed, int src, int dst) { return mpx_pattern_key(seed, (unsigned)src, (unsigned)dst, 0); }
inline uint64_t key_of(uint64_t base, int iter) { return base ^ ((uint64_t)(unsigned)iter << 24); }

// the n bytes of the pattern, written to p (any alignment)
inline void pattern(unsigned char* p, size_t n, uint64_t key) {
    size_t k = 0;
    for (; 8 * k + 8 <= n; ++k) {
        const uint64_t w = fill_word(key, k);
        memcpy(p + 8 * k, &w, 8);
    }
    if (8 * k < n) {
        const uint64_t w = fill_word(key, k);
        for (size_t b = 0; 8 * k + b < n; ++b) p[8 * k + b] = (unsigned char)(w >> (8 * b));
    }
}

// mpx_checksum's value of those n bytes, without writing them anywhere: the
// sum over the zero-padded little-endian words w_k of mix64(w_k + (k + 1) *
// golden), finished with ^ mix64(n)
inline uint64_t expect(uint64_t key, size_t n) {
    uint64_t sum = 0;
    size_t k = 0;
    for (; 8 * k + 8 <= n; ++k) sum += mix64(fill_word(key, k) + (k + 1) * kGolden);
    if (8 * k < n) {
        const uint64_t w = fill_word(key, k) & ((1ull << (8 * (n - 8 * k))) - 1);   // 1 to 7 bytes
        sum += mix64(w + (k + 1) * kGolden);
    }
    return sum ^ mix64((uint64_t)n);
}

}  // namespace seq
}  // namespace mpx
