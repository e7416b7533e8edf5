// segtree.hip -- prioritized experience replay: the sum tree, priority-proportional sampling, priorities and IS weights.
//
// Replaces the three jitted functions of /root/reference/tianshou/data/utils/segtree.py (`_setitem` :95-101, `_reduce`
// :104-116, `_get_prefix_sum_idx` :119-134) and the priority arithmetic of tianshou/data/buffer/prio.py:46-90, 103-106.
//
// The tree is the reference's, bit for bit: double tree[2 * bound], bound = the smallest power of two >= size, leaf i at
// tree[bound + i], node k = tree[2k] + tree[2k + 1] (that operand order), tree[1] the total, padding leaves 0, tree[0] unused.
//
// Set (one launch, ONE workgroup): duplicates resolve as numpy's `tree[index] = value` does -- the LAST occurrence wins.  Every
// entry i claims its leaf with atomicMax(mark[leaf], i) (mark: i32 [bound], -1 between calls); after a barrier only the entry
// that holds the claim stores, so the winner does not depend on which lane stored last.  Then the ancestors, one level per
// barrier: at level s every entry recomputes tree[p] = tree[2p] + tree[2p + 1] for p = (bound + leaf) >> s.  Both children
// are final (they belong to the level below, finished before the barrier); entries that share p store the same bits.
// log2(bound) barriers, n * log2(bound) adds: n is a sample batch or the rows of one vector step.
// An index outside [0, size) is skipped and raises the error word (tsm_segtree_check reports it); nothing faults.
//
// Sample: draw i takes words 0 and 1 of Philox4x32-10 at (seed, offset + *offset_dev + i), u = (52 bits) * 2^-52 in
// [0, 1 - 2^-52], value = u * tree[1], then the descent.  value < tree[1] ALWAYS: the exact product lies tree[1] * 2^-52 below
// tree[1], which is at least one spacing of doubles at tree[1], so rounding cannot reach tree[1] (a 53-bit u could, at a
// tie).  Hence no draw descends into a zero-weight padding leaf and nothing is clamped.
#include "common.h"
#include "philox.h"

namespace {
constexpr int kSThreads = 256;   // one thread per value / draw
constexpr int kSetMax = 1024;    // the one workgroup of the set and of the IS weights
constexpr float kEpsF32 = 1.1920928955078125e-07f;  // np.finfo(np.float32).eps (prio.py:42)

enum { SET_VALUE = 0, SET_TD = 1, SET_INIT = 2 };

__device__ __forceinline__ int64_t descend(const double *__restrict__ tree, int64_t bound, double v) {
    int64_t k = 1;
    while (k < bound) {  // segtree.py:127-132: direct = sums[2k] < value (strict); value -= lsons * direct
        k *= 2;
        const double l = tree[k];
        if (l < v) { v -= l; k += 1; }
    }
    return k - bound;
}

// x ** alpha in float32, as `np.float32 ** python float` (numpy 2 keeps f32).  alpha == 1 returns x itself: x ** 1 is x
// exactly, which a generic powf only promises to within its rounding error.
__device__ __forceinline__ float pow_alpha(float x, float alpha) { return alpha == 1.0f ? x : powf(x, alpha); }

template <int MODE>
__global__ __launch_bounds__(kSetMax) void segtree_set_kernel(double *tree, int32_t *mark, int64_t bound, int64_t size,
                                                              const int64_t *__restrict__ index, int64_t n,
                                                              const double *__restrict__ value, int64_t value_n,
                                                              const float *__restrict__ td, float alpha, double *prio,
                                                              int64_t *err) {
    __shared__ float s_hi[kSetMax / kWave], s_lo[kSetMax / kWave];
    const int t = threadIdx.x, nt = blockDim.x;
    for (int64_t i = t; i < n; i += nt) {
        const int64_t leaf = index[i];
        if (leaf < 0 || leaf >= size) { *err = 1; continue; }
        atomicMax(&mark[leaf], (int32_t)i);
    }
    __syncthreads();
    // init_weight (prio.py:46-47): max_prio ** alpha -- max_prio is 1.0 or a float32 that update_weight folded in
    const double init_leaf = MODE == SET_INIT ? (double)pow_alpha((float)prio[0], alpha) : 0.0;
    float hi = 0.f, lo = INFINITY;
    for (int64_t i = t; i < n; i += nt) {
        const int64_t leaf = index[i];
        if (leaf < 0 || leaf >= size) continue;
        double v;
        if (MODE == SET_TD) {  // prio.py:87-88 in float32
            const float w = fabsf(td[i]) + kEpsF32;
            hi = fmaxf(hi, w);
            lo = fminf(lo, w);
            v = (double)pow_alpha(w, alpha);
        } else if (MODE == SET_INIT) {
            v = init_leaf;
        } else {
            v = value[value_n == 1 ? 0 : i];
        }
        // (read where the atomics landed, in L2: an atomic does not update a line the CU's vector cache may hold)
        if (__hip_atomic_load(&mark[leaf], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int32_t)i) tree[bound + leaf] = v;
    }
    __syncthreads();
    for (int64_t i = t; i < n; i += nt) {  // withdraw the claims (every entry of a leaf stores the same -1)
        const int64_t leaf = index[i];
        if (leaf >= 0 && leaf < size) mark[leaf] = -1;
    }
    int shift = 0;
    for (int64_t width = bound; width > 1; width >>= 1) {
        ++shift;
        for (int64_t i = t; i < n; i += nt) {
            const int64_t leaf = index[i];
            if (leaf < 0 || leaf >= size) continue;
            const int64_t p = (bound + leaf) >> shift;
            tree[p] = tree[2 * p] + tree[2 * p + 1];
        }
        __syncthreads();
    }
    if (MODE == SET_TD) {  // prio.py:89-90: max / min do not depend on the order, so one workgroup-wide fold is exact
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            hi = fmaxf(hi, __shfl_xor(hi, off, kWave));
            lo = fminf(lo, __shfl_xor(lo, off, kWave));
        }
        if ((t & (kWave - 1)) == 0) { s_hi[t / kWave] = hi; s_lo[t / kWave] = lo; }
        __syncthreads();
        if (t == 0) {
            for (int k = 1; k < (nt + kWave - 1) / kWave; ++k) { hi = fmaxf(hi, s_hi[k]); lo = fminf(lo, s_lo[k]); }
            if (hi > 0.f) {  // at least one entry was in range
                prio[0] = fmax(prio[0], (double)hi);
                prio[1] = fmin(prio[1], (double)lo);
            }
        }
    }
}

__global__ __launch_bounds__(kSThreads) void segtree_prefix_kernel(const double *__restrict__ tree, int64_t bound,
                                                                   const double *__restrict__ value, int64_t n,
                                                                   int64_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kSThreads + threadIdx.x;
    if (i < n) out[i] = descend(tree, bound, value[i]);
}

__global__ void segtree_reduce_kernel(const double *__restrict__ tree, int64_t start, int64_t end, double *__restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double result = 0.0;  // segtree.py:108-116: nodes in (start, end), the additions in the reference's order
    while (end - start > 1) {
        if (start % 2 == 0) result += tree[start + 1];
        start /= 2;
        if (end % 2 == 1) result += tree[end - 1];
        end /= 2;
    }
    *out = result;
}

__global__ __launch_bounds__(kSThreads) void per_sample_kernel(const double *__restrict__ tree, int64_t bound, int64_t n,
                                                               uint64_t seed, uint64_t offset,
                                                               const uint64_t *__restrict__ offset_dev,
                                                               int64_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kSThreads + threadIdx.x;
    if (i >= n) return;
    uint32_t bits[4];
    tsm_philox4(seed, offset + (offset_dev ? *offset_dev : 0ull) + (uint64_t)i, bits);
    const uint64_t k = ((uint64_t)bits[0] << 20) | (uint64_t)(bits[1] >> 12);     // 52 bits
    const double u = (double)k * (1.0 / 4503599627370496.0);                      // [0, 1 - 2^-52]
    out[i] = descend(tree, bound, u * tree[1]);
}

// (tree[bound + idx] / min_prio) ** (-beta) in float64 (prio.py:79), divided by the batch maximum when weight_norm (:106).
__global__ __launch_bounds__(kSetMax) void per_get_weight_kernel(const double *__restrict__ tree, int64_t bound, int64_t size,
                                                                 const int64_t *__restrict__ index, int64_t n, double beta,
                                                                 int weight_norm, const double *__restrict__ prio,
                                                                 float *__restrict__ out32, double *__restrict__ out64,
                                                                 int64_t *err) {
    __shared__ double s_max[kSetMax / kWave];
    const int t = threadIdx.x, nt = blockDim.x;
    const double min_prio = prio[1];
    double hi = -INFINITY;
    int bad = 0;
    for (int64_t i = t; i < n; i += nt) {
        const int64_t leaf = index[i];
        double w;
        if (leaf < 0 || leaf >= size) {
            *err = 1;
            w = __builtin_nan("");
        } else {
            w = pow(tree[bound + leaf] / min_prio, -beta);
        }
        bad |= (w != w);
        hi = fmax(hi, w);
        out64[i] = w;
    }
    if (!weight_norm) {
        for (int64_t i = t; i < n; i += nt) out32[i] = (float)out64[i];   // (each thread reads back what it stored itself)
        return;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        hi = fmax(hi, __shfl_xor(hi, off, kWave));
        bad |= __shfl_xor(bad, off, kWave);
    }
    if ((t & (kWave - 1)) == 0) s_max[t / kWave] = bad ? __builtin_nan("") : hi;
    __syncthreads();
    double m = s_max[0];
    for (int k = 1; k < (nt + kWave - 1) / kWave; ++k) {   // np.max: a NaN weight makes the maximum NaN
        const double x = s_max[k];
        m = (m != m || x != x) ? __builtin_nan("") : fmax(m, x);
    }
    for (int64_t i = t; i < n; i += nt) {
        const double w = out64[i] / m;
        out64[i] = w;
        out32[i] = (float)w;
    }
}

int64_t bound_of(int64_t size) {
    int64_t bound = 1;
    while (bound < size) bound *= 2;
    return bound;
}

constexpr int64_t kMaxSize = (int64_t)1 << 30;  // 2 * bound doubles: 16 GB of tree at the limit

int check_tree(const char *who, const void *tree, int64_t size) {
    TSM_REQUIRE(size >= 1 && size <= kMaxSize, "%s: size = %lld outside [1, 2^30]", who, (long long)size);
    TSM_REQUIRE(tree, "%s: null pointer", who);
    return TSM_OK;
}

unsigned set_threads(int64_t n) {
    const int64_t r = ceil_div(n, kWave) * kWave;
    return (unsigned)(r < kWave ? kWave : (r > kSetMax ? kSetMax : r));
}

template <int MODE>
int launch_set(const char *who, double *tree, int32_t *mark, int64_t size, const int64_t *index, int64_t n,
               const double *value, int64_t value_n, const float *td, double alpha, double *prio, int64_t *err,
               void *stream) {
    if (int rc = check_tree(who, tree, size)) return rc;
    TSM_REQUIRE(n >= 0 && n <= INT32_MAX, "%s: n = %lld out of range", who, (long long)n);
    if (n == 0) return TSM_OK;
    TSM_REQUIRE(mark && index && err, "%s: null pointer", who);
    hipLaunchKernelGGL(segtree_set_kernel<MODE>, dim3(1), dim3(set_threads(n)), 0, tsm_stream(stream), tree, mark,
                       bound_of(size), size, index, n, value, value_n, td, (float)alpha, prio, err);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}
}  // namespace

TSM_EXPORT int64_t tsm_segtree_bound(int64_t size) {
    if (size < 1 || size > kMaxSize) return -1;
    return bound_of(size);
}

TSM_EXPORT int tsm_segtree_set(double *tree, int32_t *mark, int64_t size, const int64_t *index, int64_t n,
                               const double *value, int64_t value_n, int64_t *err, void *stream) {
    TSM_REQUIRE(value_n == 1 || value_n == n, "tsm_segtree_set: %lld values for %lld indices (one, or one each)",
                (long long)value_n, (long long)n);
    TSM_REQUIRE(n == 0 || value, "tsm_segtree_set: null pointer");
    return launch_set<SET_VALUE>("tsm_segtree_set", tree, mark, size, index, n, value, value_n, nullptr, 1.0, nullptr, err,
                                 stream);
}

TSM_EXPORT int tsm_segtree_prefix_sum_idx(const double *tree, int64_t size, const double *value, int64_t n,
                                          int64_t *index_out, void *stream) {
    if (int rc = check_tree("tsm_segtree_prefix_sum_idx", tree, size)) return rc;
    TSM_REQUIRE(n >= 0, "tsm_segtree_prefix_sum_idx: n = %lld is negative", (long long)n);
    if (n == 0) return TSM_OK;
    TSM_REQUIRE(value && index_out, "tsm_segtree_prefix_sum_idx: null pointer");
    hipLaunchKernelGGL(segtree_prefix_kernel, dim3((unsigned)ceil_div(n, kSThreads)), dim3(kSThreads), 0, tsm_stream(stream),
                       tree, bound_of(size), value, n, index_out);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_segtree_reduce(const double *tree, int64_t size, int64_t start, int64_t end, double *out, void *stream) {
    if (int rc = check_tree("tsm_segtree_reduce", tree, size)) return rc;
    TSM_REQUIRE(start >= 0 && end <= size && start <= end, "tsm_segtree_reduce: [%lld, %lld) outside [0, %lld)",
                (long long)start, (long long)end, (long long)size);
    TSM_REQUIRE(out, "tsm_segtree_reduce: null pointer");
    const int64_t bound = bound_of(size);
    hipLaunchKernelGGL(segtree_reduce_kernel, dim3(1), dim3(kWave), 0, tsm_stream(stream), tree, start + bound - 1,
                       end + bound, out);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_segtree_check(int64_t *err, void *stream) {
    TSM_REQUIRE(err, "tsm_segtree_check: null pointer");
    int64_t flag = 0;
    TSM_HIP(hipMemcpyAsync(&flag, err, sizeof(flag), hipMemcpyDeviceToHost, tsm_stream(stream)));
    TSM_HIP(hipStreamSynchronize(tsm_stream(stream)));
    if (flag) {
        TSM_HIP(hipMemsetAsync(err, 0, sizeof(flag), tsm_stream(stream)));
        tsm_set_error("segment tree: an index outside [0, size) was skipped (segtree.py:49-50)");
        return TSM_ERR_INVALID;
    }
    return TSM_OK;
}

TSM_EXPORT int tsm_per_sample(const double *tree, int64_t size, int64_t n, uint64_t seed, uint64_t offset,
                              const uint64_t *offset_dev, int64_t *index_out, void *stream) {
    if (int rc = check_tree("tsm_per_sample", tree, size)) return rc;
    TSM_REQUIRE(n >= 0, "tsm_per_sample: n = %lld is negative", (long long)n);
    if (n == 0) return TSM_OK;
    TSM_REQUIRE(index_out, "tsm_per_sample: null pointer");
    hipLaunchKernelGGL(per_sample_kernel, dim3((unsigned)ceil_div(n, kSThreads)), dim3(kSThreads), 0, tsm_stream(stream), tree,
                       bound_of(size), n, seed, offset, offset_dev, index_out);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_per_update_weight(double *tree, int32_t *mark, int64_t size, const int64_t *index, const float *td,
                                     int64_t n, double alpha, double *prio, int64_t *err, void *stream) {
    TSM_REQUIRE(alpha > 0.0, "tsm_per_update_weight: alpha = %g must be positive", alpha);
    TSM_REQUIRE(n == 0 || (td && prio), "tsm_per_update_weight: null pointer");
    return launch_set<SET_TD>("tsm_per_update_weight", tree, mark, size, index, n, nullptr, 0, td, alpha, prio, err, stream);
}

TSM_EXPORT int tsm_per_init_weight(double *tree, int32_t *mark, int64_t size, const int64_t *index, int64_t n, double alpha,
                                   double *prio, int64_t *err, void *stream) {
    TSM_REQUIRE(alpha > 0.0, "tsm_per_init_weight: alpha = %g must be positive", alpha);
    TSM_REQUIRE(n == 0 || prio, "tsm_per_init_weight: null pointer");
    return launch_set<SET_INIT>("tsm_per_init_weight", tree, mark, size, index, n, nullptr, 0, nullptr, alpha, prio, err,
                                stream);
}

TSM_EXPORT int tsm_per_get_weight(const double *tree, int64_t size, const int64_t *index, int64_t n, double beta,
                                  int weight_norm, const double *prio, float *out32, double *out64, int64_t *err,
                                  void *stream) {
    if (int rc = check_tree("tsm_per_get_weight", tree, size)) return rc;
    TSM_REQUIRE(beta >= 0.0, "tsm_per_get_weight: beta = %g is negative", beta);
    TSM_REQUIRE(n >= 0, "tsm_per_get_weight: n = %lld is negative", (long long)n);
    if (n == 0) return TSM_OK;
    TSM_REQUIRE(index && prio && out32 && out64 && err, "tsm_per_get_weight: null pointer");
    hipLaunchKernelGGL(per_get_weight_kernel, dim3(1), dim3(set_threads(n)), 0, tsm_stream(stream), tree, bound_of(size), size,
                       index, n, beta, weight_norm, prio, out32, out64, err);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}
