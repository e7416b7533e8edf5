// cql.hip -- the offline continuous learners CQL (calibrated: Cal-QL) and TD3+BC: what their updates add to csrc/cac.hip.
//
// Replaces, in tianshou/algorithm/imitation:
//   torch.FloatTensor(B R, Ad).uniform_(-min_action, max_action)                              cql.py:303-307
//   obs.unsqueeze(1).repeat(..).view(..) for obs and obs_next, and the four torch.cat([obs, act]) of the critics' inputs
//     in _calc_pi_values / _calc_random_values and current_Q                                  cql.py:218-241, 295-296, 309-319
//   F.mse_loss, the calibration torch.max, torch.cat + torch.logsumexp, the Lagrange scaling and the backward of
//     critic{1,2}_loss down to the critics' outputs                                           cql.py:299-300, 331-384
//   cql_alpha_loss.backward() and cql_alpha_optim.step()                                      cql.py:378-381
//   TD3+BC's actor loss and its backward down to the actor's raw output                       td3_bc.py:113-119
// The actor, the critics and SAC's action epilogue run in csrc/dense.hip and csrc/cac.hip.
//
// The critic row block X [(B + 3 B R)][D + Ad] stacks the data rows and the three conservative groups (uniform actions,
// policy actions at obs, policy actions at obs_next -- all three beside obs) so that each critic runs ONE forward
// and ONE backward for its whole loss.  With i a flat index in [0, B R), b = i / R, T the temperature, w the cql weight:
//   v_rand = q[B + i] - logc;  v_cur = q[B + B R + i] - logp_cur[i];  v_next = q[B + 2 B R + i] - logp_next[i]
//   with calib: each v = max(v, calib[b]) (torch.max: the gradient passes where v > calib, half of it at a tie)
//   lse_i = m + T log sum_x exp((v_x - m) / T),  m = max_x v_x     (= T logsumexp(v / T) over the THREE entries, quirk Q71)
//   cql = w mean_i lse_i - w mean_b q[b];  with the multiplier: cql_alpha = clamp(exp(log_alpha), alpha_min, alpha_max),
//   cql_scaled = cql_alpha (cql - threshold), else cql_alpha = 1 and cql_scaled = cql;  loss = mean_b (q[b] - target[b])^2 + cql_scaled
//   d loss / d q[b] = 2 (q[b] - target[b]) / B - cql_alpha w / B
//   d loss / d q[row of v_x] = cql_alpha w softmax_x((v - m) / T) pass_x / (B R)
// Every row's gradient is local given cql_alpha, which the head reads from log_alpha BEFORE tsm_cql_finalize steps it (quirk
// Q72).  All arithmetic is float64 from the float32 inputs, rounded once.  Sums: each wave's xor butterfly over its 64 indices,
// the workgroup's four waves in order, tsm_cql_finalize adds the workgroups in index order: two runs give the same bits.
#include "adam_dev.h"
#include "common.h"
#include "philox.h"
#include "q_head_dev.h"

namespace {
constexpr int kQThreads = 256;
constexpr int kQWaves = kQThreads / kWave;
constexpr uint64_t kUniformKey = 0x43514C554E49464Full;   // folded into the seed: a Philox key no other draw uses
static_assert(TSM_CQL_ROWS_PER_BLOCK == kQThreads, "one thread per flat index");
static_assert(TSM_CAC_MAX_ACT_DIM <= kWave, "one lane per action component");

// One thread per Philox block of four uniforms, the shape of cac_normal_kernel: ONE counter, the block as third counter word.
__global__ __launch_bounds__(kQThreads) void cql_uniform_kernel(float *__restrict__ out, int64_t n, float lo, float hi,
                                                                uint64_t seed, uint64_t offset,
                                                                const uint64_t *__restrict__ offset_dev) {
    const int64_t blk = (int64_t)blockIdx.x * kQThreads + threadIdx.x;
    if (blk * 4 >= n) return;
    uint32_t wd[4];
    tsm_philox4_sub(seed ^ kUniformKey, offset + (offset_dev ? *offset_dev : 0ull), (uint32_t)blk, wd);
    const float span = hi - lo;   // uniform_(from, to): u (to - from) + from, each step rounded to f32; lo == hi gives lo
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (blk * 4 + j < n) out[blk * 4 + j] = tsm_u01(wd[j]) * span + lo;
}

// Element e of X, then element e - nX of the actor rows; one float per thread and step: no alignment is asked of a row.
__global__ __launch_bounds__(kQThreads) void cql_rows_kernel(const float *__restrict__ obs, const float *__restrict__ obs_next,
                                                             const float *__restrict__ act, const float *__restrict__ rand_act,
                                                             int64_t B, int64_t R, int32_t D, int32_t Ad,
                                                             float *__restrict__ x_out, float *__restrict__ actor_rows_out) {
    const int64_t W = (int64_t)D + Ad, BR = B * R, nX = (B + 3 * BR) * W, n = nX + 2 * BR * D;
    for (int64_t e = (int64_t)blockIdx.x * kQThreads + threadIdx.x; e < n; e += (int64_t)gridDim.x * kQThreads) {
        if (e < nX) {
            const int64_t r = e / W;
            const int c = (int)(e - r * W);
            if (r < B) {
                x_out[e] = c < D ? obs[r * D + c] : act[r * Ad + (c - D)];
            } else {
                const int64_t g = (r - B) / BR, i = (r - B) - g * BR;
                if (c < D) x_out[e] = obs[(i / R) * D + c];                  // obs in all three groups (cql.py:316-319)
                else if (g == 0) x_out[e] = rand_act[i * Ad + (c - D)];      // groups 1, 2: tsm_sac_action's columns
            }
        } else {
            const int64_t e2 = e - nX, r = e2 / D;
            const int c = (int)(e2 - r * D);
            actor_rows_out[e2] = r < BR ? obs[(r / R) * D + c] : obs_next[((r - BR) / R) * D + c];
        }
    }
}

// One conservative entry: the value after the calibration max, and what of its gradient passes.
__device__ __forceinline__ double cql_calibrate(double v, const float *__restrict__ calib, int64_t b, double &pass) {
    pass = 1.0;
    if (!calib) return v;
    const double c = (double)calib[b];
    pass = v > c ? 1.0 : (v == c ? 0.5 : 0.0);
    return v > c ? v : c;
}

// Thread i < B R: the conservative group i of both critics and, where i < B, the data row i.
// partial[6 * block + {0, 1, 2}] = critic 1's {sum (q - target)^2, sum q[b], sum lse_i}, + {3, 4, 5} critic 2's.
__global__ __launch_bounds__(kQThreads) void cql_head_kernel(const float *__restrict__ q1, const float *__restrict__ q2,
                                                             const float *__restrict__ target,
                                                             const float *__restrict__ logp_cur,
                                                             const float *__restrict__ logp_next,
                                                             const float *__restrict__ calib, int64_t B, int64_t R, double logc,
                                                             double T, double wgt, double alpha_min, double alpha_max,
                                                             const float *__restrict__ log_alpha, float *__restrict__ dq1,
                                                             float *__restrict__ dq2, double *__restrict__ partial) {
    __shared__ double s_red[6][kQWaves];
    const int t = threadIdx.x, lane = t & (kWave - 1), w = t / kWave;
    const int64_t BR = B * R, i = (int64_t)blockIdx.x * TSM_CQL_ROWS_PER_BLOCK + t;
    const double ca = log_alpha ? fmin(fmax(exp((double)*log_alpha), alpha_min), alpha_max) : 1.0;
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (i < BR) {
        const int64_t b = i / R;
        const double lp[3] = {logc, (double)logp_cur[i], (double)logp_next[i]};
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const float *__restrict__ q = k ? q2 : q1;
            float *__restrict__ dq = k ? dq2 : dq1;
            double x[3], pass[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) x[j] = cql_calibrate((double)q[B + j * BR + i] - lp[j], calib, b, pass[j]);
            const double m = fmax(fmax(x[0], x[1]), x[2]);
            double e[3], s = 0.0;
#pragma unroll
            for (int j = 0; j < 3; ++j) { e[j] = exp((x[j] - m) / T); s += e[j]; }
            v[3 * k + 2] = m + T * log(s);
#pragma unroll
            for (int j = 0; j < 3; ++j) dq[B + j * BR + i] = (float)(ca * wgt * (e[j] / s) * pass[j] / (double)BR);
            if (i < B) {
                const double qd = (double)q[i], td = qd - (double)target[i];
                dq[i] = (float)(2.0 * td / (double)B - ca * wgt / (double)B);
                v[3 * k] = td * td;
                v[3 * k + 1] = qd;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const double s = wave_sum(v[k]);
        if (lane == 0) s_red[k][w] = s;
    }
    __syncthreads();
    if (t < 6) {
        double acc = 0.0;
        for (int k = 0; k < kQWaves; ++k) acc += s_red[t][k];
        partial[(int64_t)blockIdx.x * 6 + t] = acc;
    }
}

// The statistics, the multiplier's gradient and its Adam step (torch.optim.Adam's defaults but lr; the state nullable: no
// step).  One thread: the workgroups in index order.
__global__ __launch_bounds__(kWave) void cql_finalize_kernel(const double *__restrict__ partial, int64_t nb, int64_t B, int64_t BR,
                                                             double wgt, double threshold, double alpha_min, double alpha_max,
                                                             float *__restrict__ log_alpha, float *__restrict__ exp_avg,
                                                             float *__restrict__ exp_avg_sq, int64_t *__restrict__ step,
                                                             double lr, double beta1, double beta2, float eps,
                                                             float *__restrict__ out) {
    if (threadIdx.x != 0) return;
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t b = 0; b < nb; ++b)
        for (int k = 0; k < 6; ++k) s[k] += partial[6 * b + k];
    double cql[2], mse[2];
    for (int k = 0; k < 2; ++k) {
        mse[k] = s[3 * k] / (double)B;
        cql[k] = wgt * (s[3 * k + 2] / (double)BR) - wgt * (s[3 * k + 1] / (double)B);
    }
    const float nan = __builtin_nanf("");
    if (!log_alpha) {
        out[0] = (float)(mse[0] + cql[0]);
        out[1] = (float)(mse[1] + cql[1]);
        out[2] = out[3] = out[4] = out[5] = nan;
        return;
    }
    const double ea = exp((double)*log_alpha), ca = fmin(fmax(ea, alpha_min), alpha_max);
    const double excess = (cql[0] - threshold) + (cql[1] - threshold);
    const double g = (ea >= alpha_min && ea <= alpha_max) ? -0.5 * excess * ea : 0.0;   // torch.clamp's backward: inclusive
    out[0] = (float)(mse[0] + ca * (cql[0] - threshold));
    out[1] = (float)(mse[1] + ca * (cql[1] - threshold));
    out[2] = (float)ca;
    out[3] = (float)(-0.5 * ca * excess);
    out[4] = (float)g;
    float la = *log_alpha;
    if (exp_avg) {
        const int64_t k = *step + 1;
        *step = k;
        la = adam_apply(log_alpha, exp_avg, exp_avg_sq, 0, (float)g, lr, nullptr, beta1, beta2, k, nullptr, eps, 0.f, true);
    }
    out[5] = la;
}

// {sum_b |q_pi[b]|, sum_b q_pi[b]} of the whole batch in one workgroup: thread t takes rows t, t + 256, .. in order, then the
// wave butterfly and the four waves in order (a fixed order).
__global__ __launch_bounds__(kQThreads) void td3bc_qsum_kernel(const float *__restrict__ q_pi, int64_t B,
                                                               double *__restrict__ qsum) {
    __shared__ double s_red[2][kQWaves];
    const int t = threadIdx.x, lane = t & (kWave - 1), w = t / kWave;
    double a0 = 0.0, a1 = 0.0;
    for (int64_t b = t; b < B; b += kQThreads) {
        const double q = (double)q_pi[b];
        a0 += fabs(q);
        a1 += q;
    }
    a0 = wave_sum(a0);
    a1 = wave_sum(a1);
    if (lane == 0) { s_red[0][w] = a0; s_red[1][w] = a1; }
    __syncthreads();
    if (t < 2) {
        double acc = 0.0;
        for (int k = 0; k < kQWaves; ++k) acc += s_red[t][k];
        qsum[t] = acc;
    }
}

// csrc/cac.hip's shape: one wave per row, lane k holds action component k, TSM_CAC_ROWS_PER_BLOCK rows per workgroup.
// lmbda = alpha / (qsum[0] / B);  partial {sum_b (-lmbda q_pi[b] + sum_k (a - a_data)^2 / Ad), 0}.
__global__ __launch_bounds__(kQThreads) void td3bc_actor_head_kernel(const float *__restrict__ dq_da, int64_t ld,
                                                                     const float *__restrict__ omt2,
                                                                     const float *__restrict__ q_pi,
                                                                     const float *__restrict__ a, int64_t ld_a,
                                                                     const float *__restrict__ a_data, int64_t B, int32_t Ad,
                                                                     double max_action, double alpha,
                                                                     const double *__restrict__ qsum, float *__restrict__ d_raw,
                                                                     double *__restrict__ partial) {
    __shared__ double s_red[2][kQWaves];
    constexpr int kRowsPerWave = TSM_CAC_ROWS_PER_BLOCK / kQWaves;
    const int t = threadIdx.x, lane = t & (kWave - 1), w = t / kWave;
    const double lmbda = alpha / (qsum[0] / (double)B);
    double acc = 0.0;
    for (int rr = 0; rr < kRowsPerWave; ++rr) {
        const int64_t b = (int64_t)blockIdx.x * TSM_CAC_ROWS_PER_BLOCK + w * kRowsPerWave + rr;
        if (b >= B) continue;   // the whole wave leaves together
        double sq = 0.0;
        if (lane < Ad) {
            const double diff = (double)a[b * ld_a + lane] - (double)a_data[b * Ad + lane];
            sq = diff * diff;
            d_raw[b * Ad + lane] = (float)((-lmbda / (double)B * (double)dq_da[b * ld + lane] +
                                            2.0 * diff / ((double)B * (double)Ad)) * max_action * (double)omt2[b * Ad + lane]);
        }
        sq = wave_sum(sq);
        if (lane == 0) acc += -lmbda * (double)q_pi[b] + sq / (double)Ad;
    }
    tsm_store_partials(acc, 0.0, t, lane, w, s_red, partial);
}

int cql_check(const char *who, int32_t Ad, int32_t R) {
    TSM_REQUIRE(Ad >= 1 && Ad <= TSM_CAC_MAX_ACT_DIM, "%s: act_dim = %d outside [1, %d]", who, Ad, TSM_CAC_MAX_ACT_DIM);
    TSM_REQUIRE(R >= 1, "%s: num_repeat_actions should be at least 1 but got: %d", who, R);
    return TSM_OK;
}

// B (1 + 3 R) rows of at most W floats: every element index stays below 2^31
int cql_check_rows(const char *who, int64_t B, int64_t R, int64_t W) {
    TSM_REQUIRE(B >= 1 && R >= 1 && W >= 1 && R <= (1 << 20) && W <= (1 << 20) &&
                    B <= (((int64_t)1 << 31) - 1) / ((1 + 3 * R) * W),
                "%s: B = %lld rows with num_repeat = %lld and rows of %lld floats: B (1 + 3 R) W stays below 2^31", who,
                (long long)B, (long long)R, (long long)W);
    return TSM_OK;
}
}  // namespace

TSM_EXPORT int tsm_cql_check(int32_t act_dim, int32_t num_repeat) { return cql_check("tsm_cql_check", act_dim, num_repeat); }

TSM_EXPORT int tsm_cql_uniform(float *out, int64_t n, double lo, double hi, uint64_t seed, uint64_t offset,
                               const uint64_t *offset_dev, void *stream) {
    TSM_REQUIRE(n >= 0 && n < ((int64_t)1 << 33), "tsm_cql_uniform: n = %lld out of range", (long long)n);
    TSM_REQUIRE(lo <= hi, "tsm_cql_uniform: the interval [%g, %g] is empty", lo, hi);
    if (n == 0) return TSM_OK;
    TSM_REQUIRE(out, "tsm_cql_uniform: null pointer");
    hipLaunchKernelGGL(cql_uniform_kernel, dim3((unsigned)ceil_div(ceil_div(n, 4), kQThreads)), dim3(kQThreads), 0,
                       tsm_stream(stream), out, n, (float)lo, (float)hi, seed, offset, offset_dev);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_cql_rows(const float *obs, const float *obs_next, const float *act, const float *rand_act, int64_t B,
                            int32_t num_repeat, int32_t obs_dim, int32_t act_dim, float *x_out, float *actor_rows_out,
                            void *stream) {
    if (int rc = cql_check("tsm_cql_rows", act_dim, num_repeat)) return rc;
    TSM_REQUIRE(obs_dim >= 1, "tsm_cql_rows: obs_dim = %d below 1", obs_dim);
    if (int rc = cql_check_rows("tsm_cql_rows", B, num_repeat, (int64_t)obs_dim + act_dim)) return rc;
    TSM_REQUIRE(obs && obs_next && act && rand_act && x_out && actor_rows_out, "tsm_cql_rows: null pointer");
    const int64_t BR = B * num_repeat, n = (B + 3 * BR) * ((int64_t)obs_dim + act_dim) + 2 * BR * obs_dim;
    const int64_t nb = ceil_div(n, kQThreads);
    hipLaunchKernelGGL(cql_rows_kernel, dim3((unsigned)(nb < 4096 ? nb : 4096)), dim3(kQThreads), 0, tsm_stream(stream), obs,
                       obs_next, act, rand_act, B, (int64_t)num_repeat, obs_dim, act_dim, x_out, actor_rows_out);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_cql_head(const float *q1, const float *q2, const float *target, const float *logp_cur,
                            const float *logp_next, const float *calib, int64_t B, int32_t num_repeat, double log_half_pow,
                            double temperature, double cql_weight, double alpha_min, double alpha_max, const float *log_alpha,
                            float *dq1, float *dq2, double *partial, void *stream) {
    TSM_REQUIRE(num_repeat >= 1, "tsm_cql_head: num_repeat_actions should be at least 1 but got: %d", num_repeat);
    if (int rc = cql_check_rows("tsm_cql_head", B, num_repeat, 1)) return rc;
    TSM_REQUIRE(temperature > 0.0, "tsm_cql_head: temperature = %g must be positive", temperature);
    TSM_REQUIRE(alpha_min <= alpha_max, "tsm_cql_head: alpha_min = %g above alpha_max = %g", alpha_min, alpha_max);
    TSM_REQUIRE(q1 && q2 && target && logp_cur && logp_next && dq1 && dq2 && partial, "tsm_cql_head: null pointer");
    hipLaunchKernelGGL(cql_head_kernel, dim3((unsigned)ceil_div(B * num_repeat, TSM_CQL_ROWS_PER_BLOCK)), dim3(kQThreads), 0,
                       tsm_stream(stream), q1, q2, target, logp_cur, logp_next, calib, B, (int64_t)num_repeat, log_half_pow,
                       temperature, cql_weight, alpha_min, alpha_max, log_alpha, dq1, dq2, partial);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_cql_finalize(const double *partial, int64_t n_blocks, int64_t B, int32_t num_repeat, double cql_weight,
                                double lagrange_threshold, double alpha_min, double alpha_max, float *log_alpha, float *exp_avg,
                                float *exp_avg_sq, int64_t *step, double lr, double beta1, double beta2, double eps, float *out,
                                void *stream) {
    TSM_REQUIRE(n_blocks >= 1 && B >= 1 && num_repeat >= 1, "tsm_cql_finalize: n_blocks = %lld, B = %lld, num_repeat = %d: each "
                "at least 1", (long long)n_blocks, (long long)B, num_repeat);
    TSM_REQUIRE(alpha_min <= alpha_max, "tsm_cql_finalize: alpha_min = %g above alpha_max = %g", alpha_min, alpha_max);
    TSM_REQUIRE(lr >= 0.0 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0,
                "tsm_cql_finalize: bad Adam hyper-parameters (lr = %g, betas = (%g, %g), eps = %g)", lr, beta1, beta2, eps);
    TSM_REQUIRE(partial && out, "tsm_cql_finalize: null pointer");
    TSM_REQUIRE(!exp_avg || (log_alpha && exp_avg_sq && step), "tsm_cql_finalize: the Adam state comes whole, with log_alpha");
    hipLaunchKernelGGL(cql_finalize_kernel, dim3(1), dim3(kWave), 0, tsm_stream(stream), partial, n_blocks, B,
                       B * (int64_t)num_repeat, cql_weight, lagrange_threshold, alpha_min, alpha_max, log_alpha, exp_avg, exp_avg_sq,
                       step, lr, beta1, beta2, (float)eps, out);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_td3bc_actor_head(const float *dq_da, int64_t ld, const float *one_minus_tanh2, const float *q_pi,
                                    const float *act_pi, int64_t ld_a, const float *act_data, int64_t B, int32_t act_dim,
                                    double max_action, double alpha, double *qsum_work, float *d_raw_out, double *partial,
                                    void *stream) {
    TSM_REQUIRE(act_dim >= 1 && act_dim <= TSM_CAC_MAX_ACT_DIM, "tsm_td3bc_actor_head: act_dim = %d outside [1, %d]", act_dim,
                TSM_CAC_MAX_ACT_DIM);
    if (int rc = tsm_q_check_rows("tsm_td3bc_actor_head", B)) return rc;
    TSM_REQUIRE(ld >= act_dim && ld_a >= act_dim && ld <= (1 << 20) && ld_a <= (1 << 20),
                "tsm_td3bc_actor_head: row pitches (%lld, %lld) for act_dim = %d", (long long)ld, (long long)ld_a, act_dim);
    TSM_REQUIRE(dq_da && one_minus_tanh2 && q_pi && act_pi && act_data && qsum_work && d_raw_out && partial,
                "tsm_td3bc_actor_head: null pointer");
    hipLaunchKernelGGL(td3bc_qsum_kernel, dim3(1), dim3(kQThreads), 0, tsm_stream(stream), q_pi, B, qsum_work);
    TSM_LAUNCH_CHECK();
    hipLaunchKernelGGL(td3bc_actor_head_kernel, dim3((unsigned)ceil_div(B, TSM_CAC_ROWS_PER_BLOCK)), dim3(kQThreads), 0,
                       tsm_stream(stream), dq_da, ld, one_minus_tanh2, q_pi, act_pi, ld_a, act_data, B, act_dim, max_action, alpha,
                       qsum_work, d_raw_out, partial);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}
