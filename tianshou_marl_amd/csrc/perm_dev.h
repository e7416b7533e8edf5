// perm_dev.h -- one entry of a device-side minibatch permutation, for every launch that draws them: perm_kernel /
// perm_advance_kernel (perm.hip) and the spare workgroups of the persistent rollout (rollout.hip).
//
// A permutation of [0, n) is evaluated point-wise, out[i] = pi(i): a balanced 6-round Feistel network on the smallest
// even-width power-of-two domain >= n, keyed by Philox4x32-10(seed, counter + perm index), with cycle walking (re-apply
// while the image is >= n; the domain is < 4n, so < 4 applications on average).  Every entry is independent of every other,
// so who evaluates it changes no bit.
#pragma once
#include "common.h"
#include "philox.h"

// half the width of the Feistel domain of n entries (host: the launchers pass it to the kernels)
static inline int perm_half_bits(int64_t n) {
    int bits = 0;
    while (((int64_t)1 << bits) < n) ++bits;
    return bits < 2 ? 1 : (bits + 1) / 2;
}

__device__ __forceinline__ uint32_t perm_mix32(uint32_t x) {  // full-avalanche 32-bit finalizer
    x ^= x >> 16; x *= 0x7feb352dU;
    x ^= x >> 15; x *= 0x846ca68bU;
    x ^= x >> 16;
    return x;
}

// out[p][i] = pi_p(i) * scale + (p / group_size) * offset_mul
__device__ __forceinline__ void perm_point(int64_t n, int hb, uint64_t seed, uint64_t ctr, int64_t i, int p, int64_t scale,
                                           int32_t group_size, int64_t offset_mul, int64_t *__restrict__ out) {
    uint32_t k[4];
    tsm_philox4(seed, ctr + (uint64_t)p, k);
    const uint32_t mask = (1u << hb) - 1u;
    uint32_t x = (uint32_t)i;
    do {
        uint32_t l = x >> hb, r = x & mask;
#pragma unroll
        for (int round = 0; round < 6; ++round) {
            const uint32_t f = perm_mix32(r + k[round & 3] + 0x9E3779B9u * (uint32_t)(round + 1)) & mask;
            const uint32_t t = l ^ f;
            l = r;
            r = t;
        }
        x = (l << hb) | r;
    } while ((int64_t)x >= n);
    out[(int64_t)p * n + i] = (int64_t)x * scale + (int64_t)(p / group_size) * offset_mul;
}

// The request a launch with spare workgroups serves beside its own work: all n_perm permutations of one update.
struct PermReq {
    int64_t *out;                 // [n_perm][n]; NULL = no request
    const uint64_t *counter_dev;  // read, never written
    int64_t n, scale, offset_mul;
    uint64_t seed;
    int32_t n_perm, group_size, hb;
};

// Workgroup `wg` of `n_wg` spare workgroups (blockDim.x threads each) grid-strides over the request's entries.
__device__ __forceinline__ void perm_fill(const PermReq &q, int wg, int n_wg) {
    const uint64_t ctr = __hip_atomic_load(q.counter_dev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int64_t total = q.n * q.n_perm, stride = (int64_t)n_wg * blockDim.x;
    for (int64_t j = (int64_t)wg * blockDim.x + threadIdx.x; j < total; j += stride) {
        const int p = (int)(j / q.n);
        perm_point(q.n, q.hb, q.seed, ctr, j - (int64_t)p * q.n, p, q.scale, q.group_size, q.offset_mul, q.out);
    }
}
