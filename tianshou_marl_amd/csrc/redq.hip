// redq.hip -- REDQ (arXiv 2101.05982): what lies between the ensemble critic's products and an optimiser step.
//
// Replaces, in /root/reference/tianshou/algorithm/modelfree/redq.py:
//   _target_q_compute_value (the subset's min or mean of the lagged ensemble, minus alpha logp)        :254-269
//     with the last line of `_nstep_return`                                                          algorithm_base.py:796, 1213-1215
//   the ensemble's squared loss, its gradient and the priority between the forward and optimizer.step  :273-279
//   critic(obs, a).mean(dim=0) of the actor loss                                                      :287
// The ensemble runs in csrc/ensemble.hip; the actor's head is tsm_sac_actor_head (csrc/cac.hip) fed the ensemble's mean and
// its input gradient with d_out = 1 / E; the alpha step is tsm_dsac_alpha_step.
//
// Shape: q is [E][B], one thread per row b walks the members e = 0 .. E - 1 in order (consecutive threads, consecutive
// addresses for every member), TSM_REDQ_ROWS_PER_BLOCK = 256 rows per workgroup.  Arithmetic is f64 from the f32 inputs; the
// loss leaves as per-workgroup f64 pairs in tsm_qmix_mix_td's layout: the xor butterfly over a wave's rows, then the four
// waves in order.  No atomics; two runs give the same bits.
#include "common.h"
#include "q_head_dev.h"

namespace {
constexpr int kRThreads = TSM_REDQ_ROWS_PER_BLOCK;
constexpr int kRWaves = kRThreads / kWave;

// target_q = min (mode 0) or mean (mode 1) over the members in `mask`, in member order, rounded to f32; minus alpha logp in
// f32 steps as torch does (tsm_cac_target); then the n-step line
__global__ __launch_bounds__(kRThreads) void redq_target_kernel(const float *__restrict__ q, int32_t E, uint64_t mask, int mode,
                                                                int32_t n_sub, const float *__restrict__ logp,
                                                                const float *__restrict__ alpha_dev, const float *__restrict__ mc,
                                                                const float *__restrict__ gpow, const uint8_t *__restrict__ vmask,
                                                                int64_t B, float *__restrict__ returns_out) {
    const int64_t b = (int64_t)blockIdx.x * kRThreads + threadIdx.x;
    if (b >= B) return;
    float lo = INFINITY;
    double sum = 0.0;
    bool bad = false;
    for (int e = 0; e < E; ++e) {
        if (!((mask >> e) & 1ull)) continue;
        const float v = q[(int64_t)e * B + b];
        bad |= v != v;   // torch.min keeps a NaN, fminf drops it
        lo = fminf(lo, v);
        sum += (double)v;
    }
    float tq = mode == 0 ? (bad ? __builtin_nanf("") : lo) : (float)(sum / (double)n_sub);
    if (logp) tq = __fsub_rn(tq, __fmul_rn(*alpha_dev, logp[b]));
    returns_out[b] = tsm_nstep_ret(tq, vmask[b] != 0, gpow[b], mc[b]);
}

// td_e = q_e - returns in f64 and rounded once (q - returns cancels), as cac_critic_head_kernel
__global__ __launch_bounds__(kRThreads) void redq_critic_head_kernel(const float *__restrict__ q, int32_t E,
                                                                     const float *__restrict__ returns,
                                                                     const float *__restrict__ weight, int64_t B,
                                                                     float *__restrict__ dq, float *__restrict__ prio,
                                                                     double *__restrict__ partial) {
    __shared__ double s_red[2][kRWaves];
    const int t = threadIdx.x, lane = t & (kWave - 1), w = t / kWave;
    const int64_t b = (int64_t)blockIdx.x * kRThreads + t;
    double acc = 0.0;
    if (b < B) {
        const double ret = (double)returns[b], wt = weight ? (double)weight[b] : 1.0, n = (double)E * (double)B;
        double td_sum = 0.0;
        for (int e = 0; e < E; ++e) {
            const double td = (double)q[(int64_t)e * B + b] - ret;
            dq[(int64_t)e * B + b] = (float)(2.0 * td * wt / n);
            acc += td * td * wt;
            td_sum += td;
        }
        prio[b] = (float)(td_sum / (double)E);
    }
    acc = wave_sum(acc);
    tsm_store_partials(acc, 0.0, t, lane, w, s_red, partial);
}

__global__ __launch_bounds__(kRThreads) void redq_mean_q_kernel(const float *__restrict__ q, int32_t E, int64_t B,
                                                                float *__restrict__ out) {
    const int64_t b = (int64_t)blockIdx.x * kRThreads + threadIdx.x;
    if (b >= B) return;
    double s = 0.0;
    for (int e = 0; e < E; ++e) s += (double)q[(int64_t)e * B + b];
    out[b] = (float)(s / (double)E);
}

int redq_check(const char *who, int32_t E, int64_t B) {
    TSM_REQUIRE(E >= 1 && E <= TSM_ENS_MAX_MEMBERS, "%s: ensemble size %d outside [1, %d]", who, E, TSM_ENS_MAX_MEMBERS);
    return tsm_q_check_rows(who, B);   // E * B stays below 2^31
}

inline dim3 redq_grid(int64_t B) { return dim3((unsigned)ceil_div(B, kRThreads)); }
}  // namespace

TSM_EXPORT int tsm_redq_target(const float *q_next, int32_t E, uint64_t subset_mask, int32_t mode, const float *logp_next,
                               const float *alpha_dev, const float *mc, const float *gpow, const uint8_t *vmask, int64_t B,
                               float *returns_out, void *stream) {
    if (int rc = redq_check("tsm_redq_target", E, B)) return rc;
    TSM_REQUIRE(mode == TSM_REDQ_MIN || mode == TSM_REDQ_MEAN, "tsm_redq_target: mode %d is neither min (0) nor mean (1)", mode);
    const int n_sub = __builtin_popcountll(subset_mask);
    TSM_REQUIRE(n_sub >= 1 && (E == 64 || (subset_mask >> E) == 0),
                "tsm_redq_target: the subset mask 0x%llx must name at least one of the %d members and no other",
                (unsigned long long)subset_mask, E);
    TSM_REQUIRE(q_next && mc && gpow && vmask && returns_out, "tsm_redq_target: null pointer");
    TSM_REQUIRE(!logp_next || alpha_dev, "tsm_redq_target: logp_next comes with alpha_dev");
    hipLaunchKernelGGL(redq_target_kernel, redq_grid(B), dim3(kRThreads), 0, tsm_stream(stream), q_next, E, subset_mask, mode,
                       n_sub, logp_next, alpha_dev, mc, gpow, vmask, B, returns_out);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_redq_critic_head(const float *q, int32_t E, const float *returns, const float *weight, int64_t B, float *dq,
                                    float *prio, double *partial, void *stream) {
    if (int rc = redq_check("tsm_redq_critic_head", E, B)) return rc;
    TSM_REQUIRE(q && returns && dq && prio && partial, "tsm_redq_critic_head: null pointer");
    hipLaunchKernelGGL(redq_critic_head_kernel, redq_grid(B), dim3(kRThreads), 0, tsm_stream(stream), q, E, returns, weight, B,
                       dq, prio, partial);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_redq_mean_q(const float *q, int32_t E, int64_t B, float *out, void *stream) {
    if (int rc = redq_check("tsm_redq_mean_q", E, B)) return rc;
    TSM_REQUIRE(q && out, "tsm_redq_mean_q: null pointer");
    hipLaunchKernelGGL(redq_mean_q_kernel, redq_grid(B), dim3(kRThreads), 0, tsm_stream(stream), q, E, B, out);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}
