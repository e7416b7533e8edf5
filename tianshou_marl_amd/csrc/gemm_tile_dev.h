// gemm_tile_dev.h -- what the f32-MFMA GEMM kernels share (csrc/dense.hip, csrc/ensemble.hip): the tile shape, the activation
// and its derivative, the loaders that stage a 64x16 operand tile through registers into LDS, and the descriptor check.
#pragma once
#include "common.h"

namespace {

constexpr int BM = 64, BN = 64, BK = 16, LDT = BK + 2, NT = 256;  // a k tile = BK / 16 sub-tiles of 16, staged side by side
// (BK = 32 measured slower on MI355X: 29.6 % vs 34.3 % of the f32-MFMA peak on the 384-128-128-8 critic forward)
constexpr int KS = BK / 16;

__device__ __forceinline__ float act_fwd(float v, int act) {
    if (act == 1) return v > 0.f ? v : 0.f;
    if (act == 2) return tanhf(v);
    return v;
}
// derivative expressed through the activation OUTPUT y (relu: y > 0; tanh: 1 - y^2)
__device__ __forceinline__ float act_bwd(float y, int act) {
    if (act == 1) return y > 0.f ? 1.f : 0.f;
    if (act == 2) return 1.f - y * y;
    return 1.f;
}

// tile[r][k] <- src[(r0 + r) * ld + k0 + k]   (contiguous along k).  `fast` is workgroup-uniform: the whole 64x16 piece
// is in bounds and every row start is 16-B aligned -> one unconditional 16-B load per thread (the compiler can then
// issue it early and wait for it late); edge pieces take the guarded path.
__device__ __forceinline__ void load_rowmajor(const float *__restrict__ src, int64_t ld, int64_t r0, int64_t R,
                                              int64_t k0, int64_t kend, float (&v)[4], int tid, bool fast) {
    const int r = tid >> 2, k4 = (tid & 3) * 4;
    const int64_t row = r0 + r, k = k0 + k4;
    if (fast) {
        const float4 q = *reinterpret_cast<const float4 *>(src + row * ld + k);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        return;
    }
    v[0] = v[1] = v[2] = v[3] = 0.f;
    if (row >= R) return;
    const float *p = src + row * ld + k;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (k + i < kend) v[i] = p[i];
}
__device__ __forceinline__ void store_rowmajor(float *tile, const float (&v)[4], int tid, int koff) {
    const int r = tid >> 2, k4 = (tid & 3) * 4 + koff;
    // row stride 18 words (2 x odd): conflict-free operand reads on the 32-bank LDS; rows are 8-B aligned only
    *reinterpret_cast<float2 *>(tile + r * LDT + k4) = make_float2(v[0], v[1]);
    *reinterpret_cast<float2 *>(tile + r * LDT + k4 + 2) = make_float2(v[2], v[3]);
}

// tile[r][k] <- src[(k0 + k) * ld + r0 + r]   (contiguous along r); `ones_r` = index of a virtual all-ones row
__device__ __forceinline__ void load_kmajor(const float *__restrict__ src, int64_t ld, int64_t r0, int64_t R,
                                            int64_t k0, int64_t kend, int64_t ones_r, float (&v)[4], int tid, bool fast) {
    const int k = tid >> 4, r4 = (tid & 15) * 4;
    const int64_t kk = k0 + k, row = r0 + r4;
    if (fast) {
        const float4 q = *reinterpret_cast<const float4 *>(src + kk * ld + row);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        return;
    }
    v[0] = v[1] = v[2] = v[3] = 0.f;
    if (kk >= kend) return;
    const float *p = src + kk * ld + row;
    const int64_t Rdata = ones_r >= 0 ? ones_r : R;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (row + i < Rdata) v[i] = p[i];
        else if (row + i == ones_r) v[i] = 1.f;
    }
}
__device__ __forceinline__ void store_kmajor(float *tile, const float (&v)[4], int tid, int koff) {
    const int k = (tid >> 4) + koff, r4 = (tid & 15) * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) tile[(r4 + i) * LDT + k] = v[i];
}

int check_desc(const tsm_mlp_desc *d, const char *who) {
    TSM_REQUIRE(d, "%s: null descriptor", who);
    TSM_REQUIRE(d->n_layers >= 1 && d->n_layers <= TSM_MLP_MAX_LAYERS, "%s: n_layers must be in [1, %d]", who,
                TSM_MLP_MAX_LAYERS);
    TSM_REQUIRE(d->act >= 0 && d->act <= 2, "%s: act must be 0 (none), 1 (relu) or 2 (tanh)", who);
    for (int i = 0; i <= d->n_layers; ++i)
        TSM_REQUIRE(d->dims[i] >= 1 && d->dims[i] <= (1 << 20), "%s: dims[%d] = %d out of range", who, i, d->dims[i]);
    return TSM_OK;
}

}  // namespace
