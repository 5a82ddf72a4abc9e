// philox.h — Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11; Random123) and the
// dropout mask built on it, for host and device code alike: plain 32- and 64-bit integer arithmetic, no state.
//
// The mask of one dropout site over a tensor of `count` elements in row-major order of its unpadded shape, flat index f:
//   key     = (seed & 0xffffffff, seed >> 32)          seed: the site's non-negative int64
//   counter = (g & 0xffffffff, g >> 32, 0, 0)          g = f >> 2: one block serves four consecutive elements
//   word    = block[f & 3]
//   kept iff word >= thresh,  thresh = (uint32) floor(p * 2^32 + 0.5) formed on the host in double, 0 < p < 1
//   factor  = kept ? inv_keep : 0.0f,  inv_keep = (float)(1.0 / (1.0 - p))
// A kernel applies the factor as one rounded fp32 multiplication (a dropped -3.0 becomes -0.0, as x * mask * scale gives in
// torch and numpy). The mask is a function of (seed, f) alone, so the backward recomputes it and nothing is stored.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define OCM_PHILOX_FN __host__ __device__ __forceinline__
#else
#define OCM_PHILOX_FN inline
#endif

struct philox_block {
    uint32_t w[4];
};

OCM_PHILOX_FN philox_block philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)M0 * c0, p1 = (uint64_t)M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += W0;
        k1 += W1;
    }
    return philox_block{{c0, c1, c2, c3}};
}

// the four words of group g (elements 4 g .. 4 g + 3) of the site whose seed is `seed`
OCM_PHILOX_FN philox_block dropout_words(int64_t seed, uint64_t g) {
    const uint64_t s = (uint64_t)seed;
    return philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), 0u, 0u, (uint32_t)s, (uint32_t)(s >> 32));
}

OCM_PHILOX_FN float dropout_factor(uint32_t word, uint32_t thresh, float inv_keep) { return word >= thresh ? inv_keep : 0.0f; }
