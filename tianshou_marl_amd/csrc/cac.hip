// cac.hip -- the continuous-action actor-critics (DDPG, TD3, SAC): everything between a network product and an optimiser step.
//
// Replaces, in /root/reference/tianshou:
//   ContinuousActorDeterministic.forward's max_action * tanh and TD3's smoothing noise   utils/net/continuous.py:86-88, td3.py:196-199
//   ContinuousActorProbabilistic.forward's epilogue and SACPolicy.forward               continuous.py:238-247, sac.py:108-131
//   _target_q_compute_value (min of the lagged critics, minus alpha logp for SAC)        td3.py:94-102, sac.py:298-302
//     with the last line of `_nstep_return`                                             algorithm_base.py:796, 1213-1215
//   _minimize_critic_squared_loss between the forward and optimizer.step                 ddpg.py:267-285
//   actor_loss = -critic(obs, actor(obs)).mean() and its backward to the actor's output  ddpg.py:406, td3.py:216
//   SAC's actor loss and its backward, and the entropy AutoAlpha reads                   sac.py:315-326
// The actors and critics run in csrc/dense.hip, the n-step walk in csrc/nstep.hip, the alpha step in csrc/dsac.hip.
//
// Shape: one wave per row, lane k holds action component k (Ad <= TSM_CAC_MAX_ACT_DIM = 64), four rows after one another per
// wave, four waves per workgroup (TSM_CAC_ROWS_PER_BLOCK = 16).  Every sum over the action components is the xor butterfly
// wave_sum in f64 (a fixed order, not the action order), every per-workgroup sum is lane 0's f64 running sum over the wave's
// rows followed by the four waves in order.  So two runs give the same bits.  All stores are one float per lane (consecutive
// lanes, consecutive addresses): no alignment is asked of a row pointer.
//
// SAC, per row b and component k, with m = mu_raw, s = sigma_raw, z the standard normal fed in (f64 from the f32 inputs):
//   mu = M tanh(m) (unbounded: m, and M = 1);   c = clamp(s, -20, 2);   sigma = exp(c);   x = mu + sigma z;   a = tanh(x)
//   logp = sum_k (-z^2 / 2 - c - log sqrt(2 pi)) - sum_k log(1 - a^2 + eps),   eps = finfo(float32).eps
//     (Normal.log_prob at x = mu + sigma z: ((x - mu) / sigma)^2 = z^2)
//   loss_b = alpha logp - min(q1a, q2a), the critics constants.  With G[k] = d min(q1a, q2a) / d a[k]
//     = w1 dq1/da[k] + w2 dq2/da[k], (w1, w2) = (1, 0) where q1a < q2a, (0, 1) where q2a < q1a, (1/2, 1/2) at a tie
//     (torch.min's backward), and t = 1 - a^2:
//   d logp / d x = 2 a t / (t + eps)          (-z^2 / 2 does not move: autograd's two paths through x and through mu, sigma
//                                              cancel, and d(-c)/dc = -1 is what is left of log_prob's -log sigma)
//   gx = d loss_b / d x = alpha 2 a t / (t + eps) - t G
//   d loss_b / d m = gx M (1 - tanh^2 m)      (unbounded: gx)
//   d loss_b / d s = pass (gx sigma z - alpha),   pass = 1[-20 <= s <= 2] (torch.clamp's backward: inclusive)
// and the gradient of the mean over the batch is that over B.  The entropy AutoAlpha reads is -logp.
#include "common.h"
#include "philox.h"
#include "q_head_dev.h"

namespace {
constexpr int kCThreads = 256;
constexpr int kCWaves = kCThreads / kWave;
constexpr int kCRowsPerWave = TSM_CAC_ROWS_PER_BLOCK / kCWaves;
constexpr uint64_t kNormalKey = 0x4341434E4F524D4Cull;   // folded into the seed: a Philox key no other draw uses
static_assert(TSM_CAC_MAX_ACT_DIM <= kWave, "one lane per action component");
static_assert(kCRowsPerWave * kCWaves == TSM_CAC_ROWS_PER_BLOCK, "rows per workgroup");

constexpr double kSigmaMin = -20.0, kSigmaMax = 2.0;           // continuous.py:22-23
constexpr double kLogSqrt2Pi = 0.91893853320467274178;
constexpr double kEps32 = 1.1920928955078125e-07;               // np.finfo(np.float32).eps

#define CAC_ROW_LOOP(b)                                                                                       \
    for (int rr_ = 0; rr_ < kCRowsPerWave; ++rr_)                                                             \
        if (const int64_t b = (int64_t)blockIdx.x * TSM_CAC_ROWS_PER_BLOCK + w * kCRowsPerWave + rr_; b < B)

// One thread per Philox block of four normals (Box-Muller on the word pairs (0, 1) and (2, 3)), as tsm_noisy_sample.
__global__ __launch_bounds__(kCThreads) void cac_normal_kernel(float *__restrict__ z, int64_t n, uint64_t seed, uint64_t offset,
                                                               const uint64_t *__restrict__ offset_dev) {
    const int64_t blk = (int64_t)blockIdx.x * kCThreads + threadIdx.x;
    if (blk * 4 >= n) return;
    const uint64_t counter = offset + (offset_dev ? *offset_dev : 0ull);
    uint32_t wd[4];
    tsm_philox4_sub(seed ^ kNormalKey, counter, (uint32_t)blk, wd);
    float v[4];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const float u1 = (float)((wd[2 * h] >> 8) + 1u) * (1.0f / 16777216.0f);   // (0, 1]: the logarithm never sees 0
        const float r = sqrtf(-2.0f * logf(u1)), t = 6.28318530717958647692f * tsm_u01(wd[2 * h + 1]);
        v[2 * h] = r * cosf(t);
        v[2 * h + 1] = r * sinf(t);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (blk * 4 + j < n) z[blk * 4 + j] = v[j];
}

// rows_out[b][col0 + k] = M tanh(raw[b][k]) (+ clamp(policy_noise z, +-noise_clip); noise_clip <= 0: no clamp); the sum is
// NOT clamped to the action bounds (td3.py:199).  omt2 (nullable) <- 1 - tanh^2.
__global__ __launch_bounds__(kCThreads) void cac_det_action_kernel(const float *__restrict__ raw, const float *__restrict__ z,
                                                                   int64_t B, int32_t Ad, float max_action, float policy_noise,
                                                                   float noise_clip, float *__restrict__ rows_out, int64_t W,
                                                                   int32_t col0, float *__restrict__ omt2) {
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    CAC_ROW_LOOP(b) {
        if (lane < Ad) {
            const double th = tanh((double)raw[b * Ad + lane]);
            float a = __fmul_rn(max_action, (float)th);
            if (z) {
                float nz = __fmul_rn(z[b * Ad + lane], policy_noise);
                if (noise_clip > 0.f) nz = fminf(fmaxf(nz, -noise_clip), noise_clip);
                a = __fadd_rn(a, nz);
            }
            rows_out[b * W + col0 + lane] = a;
            if (omt2) omt2[b * Ad + lane] = (float)(1.0 - th * th);
        }
    }
}

// The row's SAC action: this lane's a, sigma, pass and 1 - tanh^2(mu_raw) (f64), the row's logp in every lane.
struct SacLane { double a, sigma, pass, omt2, z; };
__device__ __forceinline__ double sac_row(const float *__restrict__ mu_row, const float *__restrict__ sg_row,
                                          const float *__restrict__ z_row, int Ad, int lane, double M, bool unbounded,
                                          SacLane &o) {
    const bool in = lane < Ad;
    const double m = in ? (double)mu_row[lane] : 0.0, s = in ? (double)sg_row[lane] : 0.0;
    o.z = (in && z_row) ? (double)z_row[lane] : 0.0;   // no z: the mode
    const double th = tanh(m);
    o.omt2 = unbounded ? 1.0 : 1.0 - th * th;
    const double mu = unbounded ? m : M * th;
    o.pass = (s >= kSigmaMin && s <= kSigmaMax) ? 1.0 : 0.0;
    const double c = fmin(fmax(s, kSigmaMin), kSigmaMax);
    o.sigma = exp(c);
    o.a = tanh(mu + o.sigma * o.z);
    const double term = -0.5 * o.z * o.z - c - kLogSqrt2Pi - log(1.0 - o.a * o.a + kEps32);
    return wave_sum(in ? term : 0.0);
}

__global__ __launch_bounds__(kCThreads) void sac_action_kernel(const float *__restrict__ mu_raw, int64_t ld_mu,
                                                               const float *__restrict__ sigma_raw, int64_t ld_sigma,
                                                               const float *__restrict__ z, int64_t B, int32_t Ad,
                                                               float max_action, int unbounded, float *__restrict__ rows_out,
                                                               int64_t W, int32_t col0, float *__restrict__ logp_out) {
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    CAC_ROW_LOOP(b) {
        SacLane o;
        const double logp = sac_row(mu_raw + b * ld_mu, sigma_raw + b * ld_sigma, z ? z + b * Ad : nullptr, Ad, lane,
                                    (double)max_action, unbounded != 0, o);
        if (lane < Ad) rows_out[b * W + col0 + lane] = (float)o.a;
        if (lane == 0 && logp_out) logp_out[b] = (float)logp;
    }
}

// target_q = min(q1, q2) (q2 null: q1) - alpha logp (logp null: nothing), each step rounded to f32 as torch does; then the
// n-step line
__global__ __launch_bounds__(kCThreads) void cac_target_kernel(const float *__restrict__ q1, const float *__restrict__ q2,
                                                               const float *__restrict__ logp,
                                                               const float *__restrict__ alpha_dev, const float *__restrict__ mc,
                                                               const float *__restrict__ gpow, const uint8_t *__restrict__ vmask,
                                                               int64_t B, float *__restrict__ returns_out) {
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    CAC_ROW_LOOP(b) {
        if (lane == 0) {
            float tq = q2 ? fminf(q1[b], q2[b]) : q1[b];
            if (q2 && (q1[b] != q1[b] || q2[b] != q2[b])) tq = __builtin_nanf("");   // torch.min keeps a NaN, fminf drops it
            if (logp) tq = __fsub_rn(tq, __fmul_rn(*alpha_dev, logp[b]));
            returns_out[b] = tsm_nstep_ret(tq, vmask[b] != 0, gpow[b], mc[b]);
        }
    }
}

// td = q - returns formed in f64 from the f32 inputs and rounded once (q - returns cancels), as maddpg_td_kernel
__global__ __launch_bounds__(kCThreads) void cac_critic_head_kernel(const float *__restrict__ q1, const float *__restrict__ q2,
                                                                    const float *__restrict__ returns,
                                                                    const float *__restrict__ weight, int64_t B,
                                                                    float *__restrict__ dq1, float *__restrict__ dq2,
                                                                    float *__restrict__ prio, double *__restrict__ partial) {
    __shared__ double s_red[2][kCWaves];
    const int t = threadIdx.x, lane = t & (kWave - 1), w = t / kWave;
    double acc1 = 0.0, acc2 = 0.0;
    CAC_ROW_LOOP(b) {
        if (lane == 0) {
            const double ret = (double)returns[b], wt = weight ? (double)weight[b] : 1.0;
            const double td1 = (double)q1[b] - ret;
            dq1[b] = (float)(2.0 * td1 * wt / (double)B);
            acc1 += td1 * td1 * wt;
            double pr = td1;
            if (q2) {
                const double td2 = (double)q2[b] - ret;
                dq2[b] = (float)(2.0 * td2 * wt / (double)B);
                acc2 += td2 * td2 * wt;
                pr = (td1 + td2) / 2.0;
            }
            prio[b] = (float)pr;
        }
    }
    tsm_store_partials(acc1, acc2, t, lane, w, s_red, partial);
}

// d_raw[b][k] = -(dq_da[b][k] M omt2[b][k]) / B;  partial {sum -q_pi, 0}
__global__ __launch_bounds__(kCThreads) void cac_det_actor_head_kernel(const float *__restrict__ dq_da, int64_t ld,
                                                                       const float *__restrict__ omt2,
                                                                       const float *__restrict__ q_pi, int64_t B, int32_t Ad,
                                                                       float max_action, float *__restrict__ d_raw,
                                                                       double *__restrict__ partial) {
    __shared__ double s_red[2][kCWaves];
    const int t = threadIdx.x, lane = t & (kWave - 1), w = t / kWave;
    double acc = 0.0;
    CAC_ROW_LOOP(b) {
        if (lane < Ad)
            d_raw[b * Ad + lane] = (float)(-((double)dq_da[b * ld + lane] * (double)max_action * (double)omt2[b * Ad + lane]) /
                                           (double)B);
        if (lane == 0) acc += -(double)q_pi[b];
    }
    tsm_store_partials(acc, 0.0, t, lane, w, s_red, partial);
}

// The head comment's gradient.  Nothing is saved by tsm_sac_action: a, sigma, pass, 1 - tanh^2 and logp are formed again by
// sac_row from the actor's raw output and the same z, so they are the same f64 numbers (the critics saw a rounded to f32).
// partial {sum loss_b, sum -logp}.
__global__ __launch_bounds__(kCThreads) void sac_actor_head_kernel(const float *__restrict__ mu_raw, int64_t ld_mu,
                                                                   const float *__restrict__ sigma_raw, int64_t ld_sigma,
                                                                   const float *__restrict__ z,
                                                                   const float *__restrict__ q1a, const float *__restrict__ q2a,
                                                                   const float *__restrict__ g1, const float *__restrict__ g2,
                                                                   int64_t ld_g, const float *__restrict__ alpha_dev, int64_t B,
                                                                   int32_t Ad, float max_action, int unbounded,
                                                                   float *__restrict__ d_mu, float *__restrict__ d_sigma,
                                                                   int64_t ld_d, float *__restrict__ logp_out,
                                                                   double *__restrict__ partial) {
    __shared__ double s_red[2][kCWaves];
    const int t = threadIdx.x, lane = t & (kWave - 1), w = t / kWave;
    const double alpha = (double)*alpha_dev, M = (double)max_action;
    double acc_l = 0.0, acc_h = 0.0;
    CAC_ROW_LOOP(b) {
        const bool in = lane < Ad;
        SacLane o;
        const double logp = sac_row(mu_raw + b * ld_mu, sigma_raw + b * ld_sigma, z ? z + b * Ad : nullptr, Ad, lane, M,
                                    unbounded != 0, o);
        const double a = o.a, tt = 1.0 - a * a;
        const float qa = q1a[b], qb = q2a ? q2a[b] : qa;
        const double w1 = !q2a ? 1.0 : (qa < qb ? 1.0 : (qb < qa ? 0.0 : 0.5));
        if (in) {
            const double G = w1 * (double)g1[b * ld_g + lane] + (q2a ? (1.0 - w1) * (double)g2[b * ld_g + lane] : 0.0);
            const double gx = alpha * 2.0 * a * tt / (tt + kEps32) - tt * G;
            d_mu[b * ld_d + lane] = (float)(gx * (unbounded ? 1.0 : M) * o.omt2 / (double)B);
            d_sigma[b * ld_d + lane] = (float)(o.pass * (gx * o.sigma * o.z - alpha) / (double)B);
        }
        if (lane == 0) {
            if (logp_out) logp_out[b] = (float)logp;
            acc_l += alpha * logp - (double)fminf(qa, qb);
            acc_h += -logp;   // before the rounding to f32: the alpha step reads this sum
        }
    }
    tsm_store_partials(acc_l, acc_h, t, lane, w, s_red, partial);
}

// The gradient of a state-independent sigma row: wave k sums d[b][k] over the rows (lane l takes rows l, l + 64, ... in
// order, then the xor butterfly: a fixed order) into slab 0 of the gradient slabs and writes zero into the other slabs.
__global__ __launch_bounds__(kWave) void cac_col_sum_kernel(const float *__restrict__ d, int64_t ld, int64_t B, int32_t n_slab,
                                                            float *__restrict__ out, int64_t slab_stride) {
    const int lane = threadIdx.x, k = blockIdx.x;
    double acc = 0.0;
    for (int64_t b = lane; b < B; b += kWave) acc += (double)d[b * ld + k];
    acc = wave_sum(acc);
    if (lane < n_slab) out[(int64_t)lane * slab_stride + k] = lane == 0 ? (float)acc : 0.f;
}

int cac_check(const char *who, int32_t Ad, int32_t n_step) {
    TSM_REQUIRE(Ad >= 1 && Ad <= TSM_CAC_MAX_ACT_DIM, "%s: act_dim = %d outside [1, %d]", who, Ad, TSM_CAC_MAX_ACT_DIM);
    TSM_REQUIRE(n_step >= 1, "%s: n_step_return_horizon should be greater than 0 but got: %d", who, n_step);
    return TSM_OK;
}

// B rows of Ad components; output rows of W floats written at [col0, col0 + Ad): every index stays below 2^31 * 64
int cac_check_rows(const char *who, int64_t B, int32_t Ad) {
    if (int rc = cac_check(who, Ad, 1)) return rc;
    return tsm_q_check_rows(who, B);
}

int cac_check_out_rows(const char *who, int64_t B, int32_t Ad, int64_t W, int32_t col0) {
    if (int rc = cac_check_rows(who, B, Ad)) return rc;
    TSM_REQUIRE(col0 >= 0 && (int64_t)col0 + Ad <= W && W <= (1 << 20),
                "%s: columns [%d, %d) leave the row of %lld floats (at most 2^20)", who, col0, col0 + Ad, (long long)W);
    return TSM_OK;
}

inline dim3 cac_grid(int64_t B) { return dim3((unsigned)ceil_div(B, TSM_CAC_ROWS_PER_BLOCK)); }
}  // namespace

TSM_EXPORT int tsm_cac_check(int32_t act_dim, int32_t n_step) { return cac_check("tsm_cac_check", act_dim, n_step); }

TSM_EXPORT int tsm_cac_normal(float *z_out, int64_t n, uint64_t seed, uint64_t offset, const uint64_t *offset_dev,
                              void *stream) {
    TSM_REQUIRE(n >= 0 && n < ((int64_t)1 << 33), "tsm_cac_normal: n = %lld out of range", (long long)n);
    if (n == 0) return TSM_OK;
    TSM_REQUIRE(z_out, "tsm_cac_normal: null pointer");
    hipLaunchKernelGGL(cac_normal_kernel, dim3((unsigned)ceil_div(ceil_div(n, 4), kCThreads)), dim3(kCThreads), 0,
                       tsm_stream(stream), z_out, n, seed, offset, offset_dev);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_cac_det_action(const float *raw, const float *z, int64_t B, int32_t act_dim, double max_action,
                                  double policy_noise, double noise_clip, float *rows_out, int64_t W, int32_t col0,
                                  float *one_minus_tanh2_out, void *stream) {
    if (int rc = cac_check_out_rows("tsm_cac_det_action", B, act_dim, W, col0)) return rc;
    TSM_REQUIRE(raw && rows_out, "tsm_cac_det_action: null pointer");
    hipLaunchKernelGGL(cac_det_action_kernel, cac_grid(B), dim3(kCThreads), 0, tsm_stream(stream), raw, z, B, act_dim,
                       (float)max_action, (float)policy_noise, (float)noise_clip, rows_out, W, col0, one_minus_tanh2_out);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_sac_action(const float *mu_raw, int64_t ld_mu, const float *sigma_raw, int64_t ld_sigma, const float *z,
                              int64_t B, int32_t act_dim, double max_action, int32_t unbounded, float *rows_out, int64_t W,
                              int32_t col0, float *logp_out, void *stream) {
    if (int rc = cac_check_out_rows("tsm_sac_action", B, act_dim, W, col0)) return rc;
    TSM_REQUIRE(ld_mu >= act_dim && (ld_sigma == 0 || ld_sigma >= act_dim) && ld_mu <= (1 << 20) && ld_sigma <= (1 << 20),
                "tsm_sac_action: row pitches (%lld, %lld) for act_dim = %d (sigma: 0 = one row for all)", (long long)ld_mu,
                (long long)ld_sigma, act_dim);
    TSM_REQUIRE(mu_raw && sigma_raw && rows_out, "tsm_sac_action: null pointer");
    hipLaunchKernelGGL(sac_action_kernel, cac_grid(B), dim3(kCThreads), 0, tsm_stream(stream), mu_raw, ld_mu, sigma_raw,
                       ld_sigma, z, B, act_dim, (float)max_action, unbounded, rows_out, W, col0, logp_out);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_cac_col_sum(const float *d, int64_t ld, int64_t B, int32_t act_dim, int32_t n_slab, float *slabs_out,
                               int64_t slab_stride, void *stream) {
    if (int rc = cac_check_rows("tsm_cac_col_sum", B, act_dim)) return rc;
    TSM_REQUIRE(ld >= act_dim && ld <= (1 << 20), "tsm_cac_col_sum: row pitch %lld for act_dim = %d", (long long)ld, act_dim);
    TSM_REQUIRE(n_slab >= 1 && n_slab <= kWave && (n_slab == 1 || slab_stride >= act_dim),
                "tsm_cac_col_sum: n_slab = %d outside [1, %d] or slab pitch %lld below act_dim = %d", n_slab, kWave,
                (long long)slab_stride, act_dim);
    TSM_REQUIRE(d && slabs_out, "tsm_cac_col_sum: null pointer");
    hipLaunchKernelGGL(cac_col_sum_kernel, dim3((unsigned)act_dim), dim3(kWave), 0, tsm_stream(stream), d, ld, B, n_slab,
                       slabs_out, slab_stride);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_cac_target(const float *q1_next, const float *q2_next, const float *logp_next, const float *alpha_dev,
                              const float *mc, const float *gpow, const uint8_t *vmask, int64_t B, float *returns_out,
                              void *stream) {
    if (int rc = tsm_q_check_rows("tsm_cac_target", B)) return rc;
    TSM_REQUIRE(q1_next && mc && gpow && vmask && returns_out, "tsm_cac_target: null pointer");
    TSM_REQUIRE(!logp_next || alpha_dev, "tsm_cac_target: logp_next comes with alpha_dev");
    hipLaunchKernelGGL(cac_target_kernel, cac_grid(B), dim3(kCThreads), 0, tsm_stream(stream), q1_next, q2_next, logp_next,
                       alpha_dev, mc, gpow, vmask, B, returns_out);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_cac_critic_head(const float *q1, const float *q2, const float *returns, const float *weight, int64_t B,
                                   float *dq1, float *dq2, float *prio, double *partial, void *stream) {
    if (int rc = tsm_q_check_rows("tsm_cac_critic_head", B)) return rc;
    TSM_REQUIRE(q1 && returns && dq1 && prio && partial && (!q2 || dq2), "tsm_cac_critic_head: null pointer");
    hipLaunchKernelGGL(cac_critic_head_kernel, cac_grid(B), dim3(kCThreads), 0, tsm_stream(stream), q1, q2, returns, weight, B,
                       dq1, dq2, prio, partial);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_cac_det_actor_head(const float *dq_da, int64_t ld, const float *one_minus_tanh2, const float *q_pi,
                                      int64_t B, int32_t act_dim, double max_action, float *d_raw_out, double *partial,
                                      void *stream) {
    if (int rc = cac_check_rows("tsm_cac_det_actor_head", B, act_dim)) return rc;
    TSM_REQUIRE(ld >= act_dim && ld <= (1 << 20), "tsm_cac_det_actor_head: row pitch %lld for act_dim = %d", (long long)ld,
                act_dim);
    TSM_REQUIRE(dq_da && one_minus_tanh2 && q_pi && d_raw_out && partial, "tsm_cac_det_actor_head: null pointer");
    hipLaunchKernelGGL(cac_det_actor_head_kernel, cac_grid(B), dim3(kCThreads), 0, tsm_stream(stream), dq_da, ld,
                       one_minus_tanh2, q_pi, B, act_dim, (float)max_action, d_raw_out, partial);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_sac_actor_head(const float *mu_raw, int64_t ld_mu, const float *sigma_raw, int64_t ld_sigma,
                                  const float *z, const float *q1a, const float *q2a, const float *dq1_da, const float *dq2_da, int64_t ld_g,
                                  const float *alpha_dev, int64_t B, int32_t act_dim, double max_action, int32_t unbounded,
                                  float *d_mu_out, float *d_sigma_out, int64_t ld_d, float *logp_out, double *partial,
                                  void *stream) {
    if (int rc = cac_check_rows("tsm_sac_actor_head", B, act_dim)) return rc;
    TSM_REQUIRE(ld_mu >= act_dim && ld_g >= act_dim && ld_d >= act_dim && (ld_sigma == 0 || ld_sigma >= act_dim) &&
                    ld_mu <= (1 << 20) && ld_g <= (1 << 20) && ld_d <= (1 << 20) && ld_sigma <= (1 << 20),
                "tsm_sac_actor_head: row pitches (%lld, %lld, %lld, %lld) for act_dim = %d", (long long)ld_mu,
                (long long)ld_sigma, (long long)ld_g, (long long)ld_d, act_dim);
    TSM_REQUIRE(mu_raw && sigma_raw && q1a && dq1_da && alpha_dev && d_mu_out && d_sigma_out && partial && (!q2a || dq2_da),
                "tsm_sac_actor_head: null pointer");
    hipLaunchKernelGGL(sac_actor_head_kernel, cac_grid(B), dim3(kCThreads), 0, tsm_stream(stream), mu_raw, ld_mu, sigma_raw,
                       ld_sigma, z, q1a, q2a, dq1_da, dq2_da, ld_g, alpha_dev, B, act_dim, (float)max_action, unbounded, d_mu_out,
                       d_sigma_out, ld_d, logp_out, partial);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}
