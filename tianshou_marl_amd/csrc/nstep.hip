// nstep.hip -- the n-step walk of Algorithm.compute_nstep_return over the device buffer's index algebra.
//
// Replaces the `buffer.next` stack, `value_mask`, the end flags and `_nstep_return`
// (/root/reference/tianshou/algorithm/algorithm_base.py:773-806, 1155-1216) for all I sampled flat indices in one launch.
// What stays outside is the target network on obs_next[idx_n] (csrc/dense.hip) and the last line of `_nstep_return`,
//   returns = target_q * value_mask * gamma^m + mc,
// which the TD head (csrc/dqn.hip) evaluates from this kernel's outputs.
//
// Per index i (one thread; at most n_step dependent loads of done / reward):
//   cur_0 = indices[i], cur_{n+1} = next(cur_n)                         manager.py:334-358, as tsm_vrb_next
//   end(c) = done[c] | isin(c, unfinished_index())                      algorithm_base.py:797-798
//   f      = the first n in [0, n_step) with end(cur_n), else n_step - 1
//   mc     = sum_{n <= f} gamma^n rew[cur_n][k]     m = f + 1 if an end was met, else n_step      gpow = gamma^m
// The reference's backward loop (:1207-1211) zeroes the sum at every end flag it meets on its way down, so only the rows up
// to the first end survive: the same sum.  mc and the powers of gamma are float64 in registers (numba's types), rounded once
// on the store; gamma^m is built by repeated multiplication as `gamma_buffer_N` is (:1197-1199).
#include "common.h"
#include "vrb_dev.h"

namespace {

__global__ __launch_bounds__(256) void nstep_kernel(const void *state, int64_t B, int64_t S,
                                                    const uint8_t *__restrict__ done_store,
                                                    const uint8_t *__restrict__ term_store, int64_t term_stride,
                                                    int32_t term_col, const float *__restrict__ rew_store,
                                                    int64_t rew_stride, int32_t rew_col,
                                                    const int64_t *__restrict__ indices, int64_t I, int32_t n_step,
                                                    double gamma, int64_t *__restrict__ idx_n, float *__restrict__ mc_out,
                                                    float *__restrict__ gpow_out, uint8_t *__restrict__ vmask) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= I) return;
    VrbState s = vrb_view(const_cast<void *>(state), B, 1);  // the fields read here precede ep_return
    int64_t cur = pymod(indices[i], B * S);
    const int64_t e = cur / S, start = e * S;     // next() never leaves the sub-buffer
    int64_t cur_len = s.lengths[e];
    if (cur_len < 1) cur_len = 1;
    const int64_t last_index = s.last_index[e];
    // unfinished_index() of this sub-buffer (buffer_base.py:309-312): its newest row, unless that row ended an episode
    const int64_t sz = s.size[e];
    int64_t unfinished = -1;
    if (sz > 0) {
        const int64_t last = pymod(s.ins[e] - 1, sz);
        if (!done_store[last * B + e]) unfinished = last + start;
    }
    double mc = 0.0, g = 1.0;
    bool ended = false;
    for (int n = 0; n < n_step; ++n) {
        const int64_t sub = cur - start;
        const bool done = done_store[sub * B + e] != 0;
        if (!ended) {
            mc += g * (double)rew_store[(sub * B + e) * rew_stride + rew_col];
            g *= gamma;
            ended = done || cur == unfinished;
        }
        if (n == n_step - 1) break;
        const int64_t end_flag = (done ? 1 : 0) | (cur == last_index ? 1 : 0);
        const int64_t nxt = pymod(sub + 1 - end_flag, cur_len) + start;
        if (ended && nxt == cur) break;  // a fixed point of next(): the remaining applications change nothing
        cur = nxt;
    }
    // g = gamma^m: one multiplication per row summed -- f + 1 of them when an end was met, n_step otherwise
    const int64_t sub = cur - start;
    idx_n[i] = cur;
    mc_out[i] = (float)mc;
    gpow_out[i] = (float)g;
    vmask[i] = term_store[(sub * B + e) * term_stride + term_col] ? 0 : 1;
}

}  // namespace

TSM_EXPORT int tsm_nstep_return(const void *state, int64_t B, int64_t S, const uint8_t *done_store,
                                const uint8_t *term_store, int64_t term_row_stride, int32_t term_col,
                                const float *rew_store, int64_t rew_row_stride, int32_t rew_col, const int64_t *indices,
                                int64_t I, int32_t n_step, double gamma, int64_t *idx_n, float *mc, float *gpow,
                                uint8_t *vmask, void *stream) {
    TSM_REQUIRE(n_step >= 1, "tsm_nstep_return: n_step = %d, must be >= 1", n_step);
    TSM_REQUIRE(B >= 1 && S >= 1 && I >= 0, "tsm_nstep_return: bad sizes (buffer_num = %lld, sub_size = %lld, I = %lld)",
                (long long)B, (long long)S, (long long)I);
    TSM_REQUIRE(rew_row_stride >= 1 && rew_col >= 0 && rew_col < rew_row_stride,
                "tsm_nstep_return: reward column %d outside a row of %lld", rew_col, (long long)rew_row_stride);
    TSM_REQUIRE(term_row_stride >= 1 && term_col >= 0 && term_col < term_row_stride,
                "tsm_nstep_return: terminated column %d outside a row of %lld", term_col, (long long)term_row_stride);
    TSM_REQUIRE(gamma >= 0.0 && gamma <= 1.0, "tsm_nstep_return: discount factor should be in [0, 1] but got: %g", gamma);
    if (I == 0) return TSM_OK;
    TSM_REQUIRE(state && done_store && term_store && rew_store && indices && idx_n && mc && gpow && vmask,
                "tsm_nstep_return: null pointer");
    hipLaunchKernelGGL(nstep_kernel, dim3((unsigned)ceil_div(I, 256)), dim3(256), 0, tsm_stream(stream), state, B, S,
                       done_store, term_store, term_row_stride, term_col, rew_store, rew_row_stride, rew_col, indices, I,
                       n_step, gamma, idx_n, mc, gpow, vmask);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}
