// dsac.hip -- Discrete SAC: the soft n-step target, both critic losses, the actor loss with its backward, the alpha step.
//
// Replaces DiscreteSAC._target_q_compute_value (/root/reference/tianshou/algorithm/modelfree/discrete_sac.py:147-155) with
// the last line of `_nstep_return` (algorithm_base.py:1213-1215), the arithmetic of DiscreteSAC._update_with_batch between
// the network forwards and the optimisers' steps (discrete_sac.py:162-184), and AutoAlpha.update (sac.py:203-209).  The
// actor and the critics run in csrc/dense.hip, the n-step walk in csrc/nstep.hip.
//
// Shape: one wave per row, lane a holds action a (n_act <= 64), kRowsPerWave rows after one another, 4 waves per
// workgroup.  Every sum over actions is the xor butterfly wave_sum, every per-workgroup sum is lane 0's f64 running sum
// over the wave's rows followed by the four waves in order.  So two runs give the same bits.
//
// Per row b, with x = logits[b], as torch's Categorical(logits=x):
//   ln[a] = x[a] - logsumexp(x);   p[a] = exp(x[a] - max) / sum;   H = -sum_a p[a] ln[a]   (in f64: wave_categorical)
//   (Categorical.entropy clamps ln at finfo.min before the product so that p = 0 gives 0 and not NaN.  p = 0 needs a logit
//    of -inf: finite logits give ln > -104 + (min - max) and a positive or denormal p, so the clamp is never reached and
//    the kernels do not branch on it.)
// target:  V = sum_a p[a] min(q1[b][a], q2[b][a]);   tq = V + alpha H;   returns = (float)((double)(tq vmask) gpow + mc)
//          (tsm_nstep_ret: numpy's f32 * f64 + f64, rounded once)
// critics: td_i = q_i[b][act] - returns;   l_i = td_i^2 w;   d q_i[b][act] = 2 td_i w / B;   prio = (td_1 + td_2) / 2
//          (the reference's sign, the opposite of the DQN head's td_error; a prioritized buffer takes |.|)
// actor:   loss_b = -(alpha H + V) with q1, q2 constants.  With dp[a]/dx[j] = p[a] (1[a = j] - p[j]):
//            dV/dx[j] = p[j] (q[j] - V)
//            dH/dx[j] = -sum_a p[a] (1[a = j] - p[j]) ln[a] - sum_a p[a] (1[a = j] - p[j]) = -p[j] (ln[j] + H)
//          so  d (mean_b loss_b) / d x[j] = p[j] (alpha (ln[j] + H) - (q[j] - V)) / B
// An action outside [0, n_act) reads nothing: the row's prio and loss terms are NaN and its gradient zero, as in the DQN
// and distributional heads.  Losses leave as per-workgroup f64 partials in tsm_qmix_mix_td's layout for tsm_qmix_finalize.
#include "adam_dev.h"
#include "common.h"
#include "q_head_dev.h"

namespace {
constexpr int kSThreads = 256;
constexpr int kSWaves = kSThreads / kWave;
constexpr int kSRowsPerWave = TSM_DSAC_ROWS_PER_BLOCK / kSWaves;
static_assert(kQHeadMaxA <= kWave, "one lane per action");
static_assert(kSRowsPerWave * kSWaves == TSM_DSAC_ROWS_PER_BLOCK, "rows per workgroup");

// Categorical(logits = row): this lane's probability and normalised logit (0 past A), the row's entropy in every lane.
// exp, log and the sums run in f64.  The f32 forms (expf / logf to about an ulp) are not enough for the alpha step: an
// exploring policy sits near the uniform row, where sum exp is nearly the same number in every row, so logf's error has one
// sign across the batch and stays in the MEAN entropy (1e-7 measured on an MI355X at H = 1.60), which AutoAlpha takes from a
// target a few 1e-2 away.  The cost of one f64 exp per lane and one f64 log per row has not been measured.
__device__ __forceinline__ void wave_categorical(const float *__restrict__ row, int A, int lane, double &p, double &ln,
                                                 double &H) {
    const bool in = lane < A;
    const float x = in ? row[lane] : -INFINITY;
    const float mx = wave_max(x);
    const double t = in ? (double)x - (double)mx : 0.0;
    const double e = in ? exp(t) : 0.0;
    const double s = wave_sum(e);
    ln = in ? t - log(s) : 0.0;
    p = e / s;
    H = -wave_sum(p * ln);
}

__global__ __launch_bounds__(kSThreads) void dsac_target_kernel(const float *__restrict__ logits_next,
                                                                const float *__restrict__ q1, const float *__restrict__ q2,
                                                                const float *__restrict__ alpha_dev,
                                                                const float *__restrict__ mc, const float *__restrict__ gpow,
                                                                const uint8_t *__restrict__ vmask, int64_t B, int32_t A,
                                                                float *__restrict__ returns_out) {
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    const float alpha = *alpha_dev;
    for (int rr = 0; rr < kSRowsPerWave; ++rr) {
        const int64_t b = (int64_t)blockIdx.x * TSM_DSAC_ROWS_PER_BLOCK + w * kSRowsPerWave + rr;
        if (b >= B) return;
        double p, ln, H;
        wave_categorical(logits_next + b * A, A, lane, p, ln, H);
        const float q = lane < A ? fminf(q1[b * A + lane], q2[b * A + lane]) : 0.f;
        const float tq = (float)(wave_sum(p * (double)q) + (double)alpha * H);
        if (lane == 0) returns_out[b] = tsm_nstep_ret(tq, vmask[b] != 0, gpow[b], mc[b]);
    }
}

__global__ __launch_bounds__(kSThreads) void dsac_critic_head_kernel(const float *__restrict__ q1, const float *__restrict__ q2,
                                                                     const int64_t *__restrict__ act,
                                                                     const float *__restrict__ returns,
                                                                     const float *__restrict__ weight, int64_t B, int32_t A,
                                                                     float *__restrict__ dq1, float *__restrict__ dq2,
                                                                     float *__restrict__ prio, double *__restrict__ partial) {
    __shared__ double s_red[2][kSWaves];
    const int t = threadIdx.x, lane = t & (kWave - 1), w = t / kWave;
    double acc1 = 0.0, acc2 = 0.0;
    for (int rr = 0; rr < kSRowsPerWave; ++rr) {
        const int64_t b = (int64_t)blockIdx.x * TSM_DSAC_ROWS_PER_BLOCK + w * kSRowsPerWave + rr;
        if (b >= B) break;
        const int64_t ac = act[b];
        const bool ok = ac >= 0 && ac < A;   // an action outside [0, A) reads nothing and poisons the losses
        const float nanv = __builtin_nanf("");
        const float ret = returns[b], wt = weight ? weight[b] : 1.f;
        const float td1 = (ok ? q1[b * A + ac] : nanv) - ret, td2 = (ok ? q2[b * A + ac] : nanv) - ret;
        const float g1 = 2.f * td1 * wt / (float)B, g2 = 2.f * td2 * wt / (float)B;
        if (lane < A) {
            const bool hit = ok && lane == (int)ac;
            dq1[b * A + lane] = hit ? g1 : 0.f;
            dq2[b * A + lane] = hit ? g2 : 0.f;
        }
        if (lane == 0) {
            prio[b] = (td1 + td2) / 2.f;
            acc1 += (double)(td1 * td1 * wt);
            acc2 += (double)(td2 * td2 * wt);
        }
    }
    tsm_store_partials(acc1, acc2, t, lane, w, s_red, partial);
}

__global__ __launch_bounds__(kSThreads) void dsac_actor_head_kernel(const float *__restrict__ logits,
                                                                    const float *__restrict__ q1, const float *__restrict__ q2,
                                                                    const float *__restrict__ alpha_dev, int64_t B, int32_t A,
                                                                    float *__restrict__ entropy, float *__restrict__ d_logits,
                                                                    double *__restrict__ partial) {
    __shared__ double s_red[2][kSWaves];
    const int t = threadIdx.x, lane = t & (kWave - 1), w = t / kWave;
    const float alpha = *alpha_dev;
    double acc_l = 0.0, acc_h = 0.0;
    for (int rr = 0; rr < kSRowsPerWave; ++rr) {
        const int64_t b = (int64_t)blockIdx.x * TSM_DSAC_ROWS_PER_BLOCK + w * kSRowsPerWave + rr;
        if (b >= B) break;
        double p, ln, H;
        wave_categorical(logits + b * A, A, lane, p, ln, H);
        const double q = lane < A ? (double)fminf(q1[b * A + lane], q2[b * A + lane]) : 0.0;
        const double V = wave_sum(p * q);
        if (lane < A) d_logits[b * A + lane] = (float)(p * ((double)alpha * (ln + H) - (q - V)) / (double)B);
        if (lane == 0) {
            entropy[b] = (float)H;
            acc_l += -((double)alpha * H + V);
            acc_h += H;   // before the rounding to f32: the alpha step reads this sum
        }
    }
    tsm_store_partials(acc_l, acc_h, t, lane, w, s_red, partial);
}

// AutoAlpha.update on device scalars: one wave.  The mean entropy is formed in f64 from the actor head's partials (lane l takes
// workgroups l, l + 64, ..., then the xor butterfly: a fixed order) and is NOT rounded to f32 before it is taken
// from the target entropy: near the target the deficit is a small difference of two numbers of the entropy's size, and one
// f32 ulp of the mean is several 1e-6 of it.  torch's single-tensor Adam through adam_apply (csrc/adam_dev.h), with 1 - beta
// formed in f64 as FlatAdam(coef64=True) has it.
__global__ __launch_bounds__(kWave) void dsac_alpha_step_kernel(const double *__restrict__ partial, int32_t nb, int64_t B,
                                                                float *__restrict__ log_alpha, float *__restrict__ exp_avg,
                                                                float *__restrict__ exp_avg_sq, int64_t *__restrict__ step,
                                                                double target_entropy, double lr, double beta1, double beta2,
                                                                float eps, float weight_decay, float *__restrict__ alpha_dev,
                                                                float *__restrict__ out) {
    const int lane = threadIdx.x;
    double s_h = 0.0;
    for (int i = lane; i < nb; i += kWave) s_h += partial[2 * i + 1];
    s_h = wave_sum(s_h);
    if (lane != 0) return;
    const double deficit = target_entropy - s_h / (double)B;         // entropy_deficit, sac.py:204, its mean over the rows
    const float alpha_loss = (float)(-((double)*log_alpha * deficit));   // :205 (log_alpha is one number)
    const float g = (float)(-deficit);                                // d alpha_loss / d log_alpha
    const int64_t k = *step + 1;
    *step = k;
    const float la = adam_apply(log_alpha, exp_avg, exp_avg_sq, 0, g, lr, nullptr, beta1, beta2, k, nullptr, eps, weight_decay,
                                true);
    const float alpha = expf(la);
    *alpha_dev = alpha;
    out[0] = alpha_loss;
    out[1] = alpha;
}

int dsac_check(const char *who, int32_t A, int32_t n_step) {
    if (int rc = tsm_q_check_act(who, A)) return rc;
    TSM_REQUIRE(n_step >= 1, "%s: n_step_return_horizon should be greater than 0 but got: %d", who, n_step);
    return TSM_OK;
}

int dsac_check_rows(const char *who, int64_t B, int32_t A) {
    if (int rc = tsm_q_check_act(who, A)) return rc;
    return tsm_q_check_rows(who, B);
}

inline dim3 dsac_grid(int64_t B) { return dim3((unsigned)ceil_div(B, TSM_DSAC_ROWS_PER_BLOCK)); }
}  // namespace

TSM_EXPORT int tsm_dsac_check(int32_t n_act, int32_t n_step) { return dsac_check("tsm_dsac_check", n_act, n_step); }

TSM_EXPORT int tsm_dsac_target(const float *logits_next, const float *q1_next_old, const float *q2_next_old,
                               const float *alpha_dev, const float *mc, const float *gpow, const uint8_t *vmask, int64_t B,
                               int32_t n_act, float *returns_out, void *stream) {
    if (int rc = dsac_check_rows("tsm_dsac_target", B, n_act)) return rc;
    TSM_REQUIRE(logits_next && q1_next_old && q2_next_old && alpha_dev && mc && gpow && vmask && returns_out,
                "tsm_dsac_target: null pointer");
    hipLaunchKernelGGL(dsac_target_kernel, dsac_grid(B), dim3(kSThreads), 0, tsm_stream(stream), logits_next, q1_next_old,
                       q2_next_old, alpha_dev, mc, gpow, vmask, B, n_act, returns_out);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_dsac_critic_head(const float *q1, const float *q2, const int64_t *act, const float *returns,
                                    const float *weight, int64_t B, int32_t n_act, float *dq1, float *dq2, float *prio,
                                    double *partial, void *stream) {
    if (int rc = dsac_check_rows("tsm_dsac_critic_head", B, n_act)) return rc;
    TSM_REQUIRE(q1 && q2 && act && returns && dq1 && dq2 && prio && partial, "tsm_dsac_critic_head: null pointer");
    hipLaunchKernelGGL(dsac_critic_head_kernel, dsac_grid(B), dim3(kSThreads), 0, tsm_stream(stream), q1, q2, act, returns,
                       weight, B, n_act, dq1, dq2, prio, partial);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_dsac_actor_head(const float *logits, const float *q1, const float *q2, const float *alpha_dev, int64_t B,
                                   int32_t n_act, float *entropy, float *d_logits, double *partial, void *stream) {
    if (int rc = dsac_check_rows("tsm_dsac_actor_head", B, n_act)) return rc;
    TSM_REQUIRE(logits && q1 && q2 && alpha_dev && entropy && d_logits && partial, "tsm_dsac_actor_head: null pointer");
    hipLaunchKernelGGL(dsac_actor_head_kernel, dsac_grid(B), dim3(kSThreads), 0, tsm_stream(stream), logits, q1, q2, alpha_dev,
                       B, n_act, entropy, d_logits, partial);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_dsac_alpha_step(const double *entropy_partial, int32_t n_blocks, int64_t B, float *log_alpha,
                                   float *exp_avg, float *exp_avg_sq, int64_t *step, double target_entropy, double lr,
                                   double beta1, double beta2, double eps, double weight_decay, float *alpha_dev, float *out,
                                   void *stream) {
    TSM_REQUIRE(n_blocks >= 1 && B >= 1, "tsm_dsac_alpha_step: bad sizes (n_blocks = %d, B = %lld)", n_blocks, (long long)B);
    TSM_REQUIRE(lr >= 0.0 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0,
                "tsm_dsac_alpha_step: bad Adam hyper-parameters (lr = %g, betas = (%g, %g), eps = %g)", lr, beta1, beta2, eps);
    TSM_REQUIRE(entropy_partial && log_alpha && exp_avg && exp_avg_sq && step && alpha_dev && out,
                "tsm_dsac_alpha_step: null pointer");
    hipLaunchKernelGGL(dsac_alpha_step_kernel, dim3(1), dim3(kWave), 0, tsm_stream(stream), entropy_partial, n_blocks, B,
                       log_alpha, exp_avg, exp_avg_sq, step, target_entropy, lr, beta1, beta2, (float)eps, (float)weight_decay,
                       alpha_dev, out);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}
