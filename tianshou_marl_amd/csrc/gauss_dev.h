// gauss_dev.h -- the device arithmetic of a diagonal Gaussian policy over Box actions, shared by the stand-alone kernels
// (gauss.hip) and the persistent Gaussian rollout (rollout_gauss.hip): one copy, so that a row's sample, log-probability and env
// action carry the same bits whichever kernel produced them.  The formulas are stated at the top of gauss.hip.
// A row is a group of G lanes (a power of two, at least 8), component k in lane k of the group; everything is f64 from the f32
// raw outputs.  Every function is __forceinline__ and takes its state by reference.
#pragma once
#include "common.h"
#include "philox.h"

namespace {
constexpr uint64_t kGaussKey = 0x4741555353504F4Cull;   // folded into the seed: a Philox key no other draw uses
constexpr double kSigmaMin = -20.0, kSigmaMax = 2.0;           // continuous.py:22-23
constexpr double kLogSqrt2Pi = 0.91893853320467274178;

template <int G>
__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

struct GaussLane { double mu, c, sigma, pass, dmu; };

// This lane's distribution parameters (zeros past act_dim, where nothing is read).
__device__ __forceinline__ void gauss_lane(const float *__restrict__ mu_row, const float *__restrict__ sg_row, bool cond,
                                           bool in, int k, double M, bool unbounded, GaussLane &o) {
    const double m = in ? (double)mu_row[k] : 0.0, s = in ? (double)sg_row[k] : 0.0;
    const double th = tanh(m);
    o.mu = unbounded ? m : M * th;
    o.dmu = unbounded ? 1.0 : M * (1.0 - th * th);
    o.pass = (!cond || (s >= kSigmaMin && s <= kSigmaMax)) ? 1.0 : 0.0;
    o.c = cond ? fmin(fmax(s, kSigmaMin), kSigmaMax) : s;
    o.sigma = exp(o.c);
}

// The row's logp in every lane of the group, from the action as stored (f32); z <- this lane's (a - mu) / sigma.
template <int G>
__device__ __forceinline__ double gauss_row(const GaussLane &o, float a, bool in, double &z) {
    z = in ? ((double)a - o.mu) / o.sigma : 0.0;
    return group_sum<G>(in ? -0.5 * z * z - o.c - kLogSqrt2Pi : 0.0);
}

// Element e's standard normal: word e % 4 of the Philox block whose third counter word is e / 4; Box-Muller on the word pairs
// (0, 1) and (2, 3) in f32, as cac_normal_kernel (csrc/cac.hip) -- the same draw under another key.
__device__ __forceinline__ float gauss_normal(uint64_t seed, uint64_t counter, int64_t e) {
    uint32_t wd[4];
    tsm_philox4_sub(seed ^ kGaussKey, counter, (uint32_t)(e >> 2), wd);
    const int h = (int)(e & 3) >> 1;
    const float u1 = (float)((wd[2 * h] >> 8) + 1u) * (1.0f / 16777216.0f);   // (0, 1]: the logarithm never sees 0
    const float r = sqrtf(-2.0f * logf(u1)), t = 6.28318530717958647692f * tsm_u01(wd[2 * h + 1]);
    return (e & 1) ? r * sinf(t) : r * cosf(t);
}

// map_action (algorithm_base.py:278-287) of the stored action: bound 0 none, 1 clip to [-1, 1], 2 tanh; low / high nullable
// together (no scaling), per component.
__device__ __forceinline__ float gauss_env_action(float a, int bound, const float *__restrict__ low,
                                                  const float *__restrict__ high, int k) {
    double x = (double)a;
    if (bound == 1) x = fmin(fmax(x, -1.0), 1.0);
    else if (bound == 2) x = tanh(x);
    if (low) {
        const double lo = (double)low[k], hi = (double)high[k];
        x = lo + (hi - lo) * (x + 1.0) / 2.0;
    }
    return (float)x;
}
}  // namespace
