// qargmax.h -- the greedy action of DiscreteQLearningPolicy.compute_q_value + argmax (dqn.py:140-151), shared by the DQN TD
// head (csrc/dqn.hip) and the distributional heads (csrc/distq.hip): one definition, so all of them pick the same a*.
#pragma once
#include "common.h"

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
