// q_head_dev.h -- what the value-based heads share (csrc/dqn.hip, csrc/distq.hip, csrc/iqn.hip, csrc/dsac.hip): the action
// limit and the row-range check, the greedy action of DiscreteQLearningPolicy.compute_q_value + argmax (dqn.py:140-151), the
// n-step return rule, the quantile-Huber term, the per-row walk and gradient scatter of the heads over per-row fractions and the
// workgroup's two f64 partials.  One definition each, so every head picks
// the same a* and rounds the same way, bit for bit.
#pragma once
#include "common.h"

// Actions of a Q head: one lane per action in csrc/dsac.hip, and every head's actions feed tsm_dqn_egreedy.
constexpr int kQHeadMaxA = 64;

static inline int tsm_q_check_act(const char *who, int32_t A) {
    TSM_REQUIRE(A >= 1 && A <= kQHeadMaxA, "%s: n_act = %d outside [1, %d]", who, A, kQHeadMaxA);
    return TSM_OK;
}

// B * n_act stays below 2^31 (wider rows are reached through 64-bit offsets)
static inline int tsm_q_check_rows(const char *who, int64_t B) {
    TSM_REQUIRE(B >= 1 && B <= ((int64_t)1 << 31) / kQHeadMaxA, "%s: B = %lld out of range", who, (long long)B);
    return TSM_OK;
}

// compute_q_value's offset logits.min() - logits.max() - 1 over the WHOLE tensor qn[0 .. n) (quirk Q15).  All NT threads of
// the workgroup call it; s_min / s_max hold NT / 64 floats each.  fminf / fmaxf skip a NaN where torch's min() / max() return
// it: a flag carries a NaN logit through the reduction and makes the offset NaN, as in the reference.  min and max do not
// depend on the order, so every workgroup gets the same bits.
template <int NT>
__device__ __forceinline__ float tsm_q_mask_offset(const float *__restrict__ qn, int64_t n, float *s_min, float *s_max) {
    const int t = threadIdx.x, lane = t & (kWave - 1), w = t / kWave;
    float lo = INFINITY, hi = -INFINITY;
    int bad = 0;
    for (int64_t j = t; j < n; j += NT) {
        const float v = qn[j];
        bad |= (v != v);
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, off, kWave));
        hi = fmaxf(hi, __shfl_xor(hi, off, kWave));
        bad |= __shfl_xor(bad, off, kWave);
    }
    if (lane == 0) { s_min[w] = bad ? __builtin_nanf("") : lo; s_max[w] = hi; }
    __syncthreads();
    lo = s_min[0];
    hi = s_max[0];
    bad = lo != lo;
#pragma unroll
    for (int k = 1; k < NT / kWave; ++k) {
        bad |= s_min[k] != s_min[k];
        lo = fminf(lo, s_min[k]);
        hi = fmaxf(hi, s_max[k]);
    }
    return bad ? __builtin_nanf("") : (lo - hi) - 1.0f;
}

// First argmax over a of row[a] + (1 - mrow[a]) * mv (mrow == nullptr: of row[a]).
__device__ __forceinline__ int tsm_q_first_argmax(const float *__restrict__ row, const uint8_t *__restrict__ mrow, int A,
                                                  float mv) {
    int a_star = 0;
    float best = 0.f;
    for (int a = 0; a < A; ++a) {
        float v = row[a];
        if (mrow) v = v + (mrow[a] ? 0.f : 1.f) * mv;   // logits + (1 - mask) * min_value, in f32 as torch
        // first maximum, as torch.argmax -- which takes the first NaN for the maximum when there is one
        if (a == 0 || v > best || (v != v && best == best)) { best = v; a_star = a; }
    }
    return a_star;
}

// target_q *= value_mask (a NaN stays a NaN); returns = target_q * gamma^m + mc in float64, rounded once: numpy's
// f32 * f64 + f64, then to_torch_as (algorithm_base.py:796, 1213-1215)
__device__ __forceinline__ float tsm_nstep_ret(float x, bool vm, float gp, float mcv) {
    const float tm = vm ? x : x * 0.f;
    return (float)((double)tm * (double)gp + (double)mcv);
}

// One pairwise term of the quantile-regression loss (qrdqn.py:119-123), u = target - current, at the fraction tau:
// h = smooth_l1(u), beta 1;  kq = |tau - 1[u <= 0]|;  ls += h kq (loss), ps += |h| (priority), gs += kq clamp(u, -1, 1) (the
// gradient; the clamp keeps a NaN)
__device__ __forceinline__ void tsm_quantile_huber(float u, float tau, float &ls, float &ps, float &gs) {
    const float au = fabsf(u);
    const float h = au < 1.f ? 0.5f * u * u : au - 0.5f;
    const float kq = fabsf(tau - (u <= 0.f ? 1.f : 0.f));
    ls += h * kq;
    ps += fabsf(h);
    gs += kq * (u != u ? u : fminf(fmaxf(u, -1.f), 1.f));
}

// One row of a quantile head over per-row fractions (csrc/iqn.hip, csrc/fqf.hip), one wave per row: lane i < N holds the taken
// action's online sample c at the fraction tau, s_ret the row's Np targets, walked j = 0 .. Np - 1 in order.  All 64 lanes
// call it.  -> the row's loss (times its weight wt), priority and mean sample, and this lane's d loss / d c for a batch of B.
__device__ __forceinline__ void tsm_quantile_row(const float *s_ret, int Np, int N, int lane, float c, float tau, float wt,
                                                 int64_t B, float &l_row, float &p_row, float &q_row, float &d) {
    const bool in = lane < N;
    float ls = 0.f, ps = 0.f, gs = 0.f;
    for (int j = 0; j < Np; ++j) tsm_quantile_huber(s_ret[j] - c, tau, ls, ps, gs);
    l_row = wave_sum(in ? ls : 0.f) / (float)N * wt;
    p_row = wave_sum(in ? ps : 0.f) / (float)N;
    q_row = wave_sum(c) / (float)N;
    d = -(wt / ((float)N * (float)B)) * gs;
}

// The row's gradient drow [N][A] from the N per-sample values s_d: zero in every other action's slots (and, with ok false, in
// all of a poisoned row's).
__device__ __forceinline__ void tsm_taken_action_scatter(float *__restrict__ drow, const float *s_d, int N, int A, int64_t ac,
                                                         bool ok, int lane) {
    for (int x = lane; x < N * A; x += kWave) {
        const int i = x / A, a = x - i * A;
        drow[x] = (ok && a == (int)ac) ? s_d[i] : 0.f;
    }
}

// The workgroup's two f64 sums into partial[2 * block + {0, 1}] (tsm_qmix_mix_td's layout, read by tsm_qmix_finalize): lane 0
// of each of the W waves holds the wave's pair; thread t < 2 adds the waves 0 .. W - 1 in order.  All threads call it, with
// t = threadIdx.x, lane = t % 64, w = t / 64.
template <int W>
__device__ __forceinline__ void tsm_store_partials(double a0, double a1, int t, int lane, int w, double (*s_red)[W],
                                                   double *__restrict__ partial) {
    if (lane == 0) { s_red[0][w] = a0; s_red[1][w] = a1; }
    __syncthreads();
    if (t < 2) {
        double acc = 0.0;
        for (int k = 0; k < W; ++k) acc += s_red[t][k];
        partial[(int64_t)blockIdx.x * 2 + t] = acc;
    }
}
