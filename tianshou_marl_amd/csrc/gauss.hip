// gauss.hip -- diagonal Gaussian policies for Box actions on the on-policy learners: the sample with its log-probability, the
// log-probability and entropy of given actions, and the PPO / policy-gradient head with its closed-form backward.
//
// Replaces, in the reference's tianshou/:
//   ContinuousActorProbabilistic.forward's epilogue                                       utils/net/continuous.py:238-247
//   Independent(Normal(loc, scale), 1).sample / .mode / .log_prob / .entropy               reinforce.py:183-192, ppo.py:157-161, 182, 210
//   map_action (bounding, then scaling, of the action the env is stepped with)             algorithm_base.py:255-288
//   the policy terms of PPO._update_with_batch and A2C's, with autograd's backward down to
//     the actor's raw outputs and to sigma_param                                           ppo.py:182-196, 210-211; a2c.py:260-270
// The actor runs in csrc/dense.hip, the value term in csrc/ppo_loss.hip (loss_kind 2), GAE in csrc/gae.hip.
//
// Shape: one group of G lanes per row, G = the power of two >= act_dim, at least 8 (kernels are instantiated for 8, 16, 32, 64);
// component k in lane k of the group, so a wave carries 64 / G rows and a workgroup of four waves 256 / G rows per pass.  A
// workgroup walks the TSM_GAUSS_ROWS_PER_BLOCK rows [blockIdx.x * R, (blockIdx.x + 1) * R) pass after pass.  A row's scalars
// (its index through perm, adv, logp_old) are loaded by the group's first lane and handed round by a width-G shuffle.  Sums over
// the components are the xor butterfly over the group in f64 (a fixed order, not the component order: every lane ends with the
// same bits); a workgroup's sums are each group's running sum over its passes, then the groups in order.  No atomics, no grid
// synchronisation: two runs give the same bits.  Every store is one float per lane at consecutive addresses, so no alignment is
// asked of a row pointer.
//
// Per row and component k, in f64 from the f32 inputs (m = mu_raw, s = sigma_raw, a = the action, M = max_action):
//   mu = M tanh(m) (unbounded: m);   c = clamp(s, -20, 2) with a conditioned sigma, s itself for the state-independent row
//   (continuous.py:242-246 clamps only the former);   sigma = exp(c);   z = (a - mu) / sigma
//   logp = sum_k (-z^2 / 2 - c - log sqrt(2 pi));   entropy = sum_k (1/2 + log sqrt(2 pi) + c)
// The action is not squashed.  The sample stores a = mu + sigma z rounded to f32 and forms logp from THAT f32 number with the
// arithmetic above (one device function, gauss_row), so tsm_gauss_logp_entropy on the stored action gives the sample's bits.
// The per-row device functions (gauss_lane, gauss_row, gauss_normal, gauss_env_action) live in gauss_dev.h, which the persistent
// Gaussian rollout (rollout_gauss.hip) includes too.
//
// The head, with A the (normalised) advantage, r = exp(logp - logp_old), lo / hi = 1 -+ eps_clip:
//   kind 0: obj = min(r A, clamp(r, lo, hi) A), with dual_clip c and A < 0: max(obj, c A);   kind 1: obj = logp A
//   loss = -mean(obj) - ent_coef mean(entropy);   gl = d loss / d logp = -(d obj / d r) r / M   (kind 1: -A / M)
//   d obj / d r follows torch's backward: min / max hand the gradient to the selected term and half to each at a tie, clamp
//   passes it on the closed interval.
//   d logp / d mu = z / sigma,   d logp / d c = z^2 - 1,   d entropy / d c = 1
//   d loss / d m = gl (z / sigma) M (1 - tanh^2 m)                      (unbounded: gl z / sigma)
//   d loss / d s = pass (gl (z^2 - 1) - ent_coef / M),   pass = 1[-20 <= s <= 2] (conditioned), 1 (state-independent)
#include "common.h"
#include "gauss_dev.h"
#include "philox.h"
#include "q_head_dev.h"

namespace {
constexpr int kGThreads = 256;
constexpr int kGMaxGroups = kGThreads / 8;  // groups of a workgroup at the narrowest group width
static_assert(TSM_CAC_MAX_ACT_DIM <= kWave, "one lane per action component");
static_assert(TSM_GAUSS_ROWS_PER_BLOCK % kGMaxGroups == 0 && TSM_GAUSS_ROWS_PER_BLOCK % (kGThreads / kWave) == 0,
              "a workgroup's rows are whole passes at every group width");

// rows of a workgroup: pass p, group q -> row blockIdx.x * R + p * (256 / G) + q.  `b < B` is uniform over a group.
#define GAUSS_ROW_LOOP(b)                                                                                          \
    for (int pass_ = 0; pass_ < TSM_GAUSS_ROWS_PER_BLOCK / (kGThreads / G); ++pass_)                               \
        if (const int64_t b = (int64_t)blockIdx.x * TSM_GAUSS_ROWS_PER_BLOCK + pass_ * (kGThreads / G) + grp; b < B)

template <int G>
__device__ __forceinline__ double gauss_entropy(const GaussLane &o, bool in) {
    return group_sum<G>(in ? 0.5 + kLogSqrt2Pi + o.c : 0.0);
}

template <int G>
__global__ __launch_bounds__(kGThreads) void gauss_sample_kernel(
    const float *__restrict__ mu_raw, int64_t ld_mu, const float *__restrict__ sigma_raw, int64_t ld_sigma, int64_t B,
    int32_t Ad, float max_action, int unbounded, uint64_t seed, uint64_t offset, const uint64_t *__restrict__ offset_dev,
    int deterministic, int bound, const float *__restrict__ low, const float *__restrict__ high, float *__restrict__ act_out,
    float *__restrict__ logp_out, float *__restrict__ env_act_out) {
    const int k = threadIdx.x % G, grp = threadIdx.x / G;
    const bool in = k < Ad, cond = ld_sigma != 0;
    const uint64_t counter = deterministic ? 0ull : offset + (offset_dev ? *offset_dev : 0ull);
    GAUSS_ROW_LOOP(b) {
        GaussLane o;
        gauss_lane(mu_raw + b * ld_mu, sigma_raw + b * ld_sigma, cond, in, k, (double)max_action, unbounded != 0, o);
        const double zn = (in && !deterministic) ? (double)gauss_normal(seed, counter, b * Ad + k) : 0.0;
        const float a = (float)(o.mu + o.sigma * zn);   // the mode draws nothing: mu
        double z;
        const double logp = gauss_row<G>(o, a, in, z);
        if (in) {
            act_out[b * Ad + k] = a;
            if (env_act_out) env_act_out[b * Ad + k] = gauss_env_action(a, bound, low, high, k);
        }
        if (k == 0 && logp_out) logp_out[b] = (float)logp;
    }
}

template <int G>
__global__ __launch_bounds__(kGThreads) void gauss_logp_entropy_kernel(
    const float *__restrict__ mu_raw, int64_t ld_mu, const float *__restrict__ sigma_raw, int64_t ld_sigma,
    const float *__restrict__ act, const int64_t *__restrict__ perm, int64_t B, int32_t Ad, float max_action, int unbounded,
    float *__restrict__ logp_out, float *__restrict__ ent_out) {
    const int k = threadIdx.x % G, grp = threadIdx.x / G;
    const bool in = k < Ad, cond = ld_sigma != 0;
    GAUSS_ROW_LOOP(b) {
        int64_t row = 0;
        if (k == 0) row = perm ? perm[b] : b;
        row = __shfl(row, 0, G);
        GaussLane o;
        gauss_lane(mu_raw + b * ld_mu, sigma_raw + b * ld_sigma, cond, in, k, (double)max_action, unbounded != 0, o);
        double z;
        const double logp = gauss_row<G>(o, in ? act[row * Ad + k] : 0.f, in, z);
        const double ent = gauss_entropy<G>(o, in);
        if (k == 0) {
            logp_out[b] = (float)logp;
            if (ent_out) ent_out[b] = (float)ent;
        }
    }
}

struct GaussCfg {
    double eps_clip, dual_clip, ent_coef;
    int adv_norm, kind;
};

template <int G>
__global__ __launch_bounds__(kGThreads) void gauss_ppo_head_kernel(
    const float *__restrict__ mu_raw, int64_t ld_mu, const float *__restrict__ sigma_raw, int64_t ld_sigma,
    const float *__restrict__ act, const float *__restrict__ logp_old, const float *__restrict__ adv,
    const int64_t *__restrict__ perm, int64_t first_row, int64_t B, int32_t Ad, const float *__restrict__ adv_stats,
    GaussCfg cfg, float max_action, int unbounded, float *__restrict__ d_mu, float *__restrict__ d_sigma, int64_t ld_d,
    double *__restrict__ partial, double *__restrict__ col_partial) {
    __shared__ double s_red[2][kGMaxGroups];
    __shared__ double s_col[kGThreads];
    const int k = threadIdx.x % G, grp = threadIdx.x / G;
    const bool in = k < Ad, cond = ld_sigma != 0;
    const double invM = 1.0 / (double)B;
    double mean = 0.0, istd = 1.0;
    if (cfg.adv_norm) {   // (ppo.py:185: (adv - mean) / (std + self._eps), the statistics being tsm_ppo_adv_stats' f32 pair)
        mean = (double)adv_stats[0];
        istd = 1.0 / ((double)adv_stats[1] + 1e-8);
    }
    double acc_obj = 0.0, acc_ent = 0.0, acc_col = 0.0;
    GAUSS_ROW_LOOP(b) {
        // the row's scalars: loaded by the group's first lane, handed round in registers
        int64_t row = 0;
        float adv_f = 0.f, lpo_f = 0.f;
        if (k == 0) {
            row = perm ? perm[b] : first_row + b;
            adv_f = adv[row];
            lpo_f = cfg.kind == 0 ? logp_old[row] : 0.f;
        }
        row = __shfl(row, 0, G);
        const double A = ((double)__shfl(adv_f, 0, G) - mean) * istd, lpo = (double)__shfl(lpo_f, 0, G);
        GaussLane o;
        gauss_lane(mu_raw + b * ld_mu, sigma_raw + b * ld_sigma, cond, in, k, (double)max_action, unbounded != 0, o);
        double z;
        const double logp = gauss_row<G>(o, in ? act[row * Ad + k] : 0.f, in, z);
        const double ent = gauss_entropy<G>(o, in);
        double obj, g_logp;   // d obj / d logp
        if (cfg.kind == 1) {
            obj = logp * A;
            g_logp = A;
        } else {
            const double r = exp(logp - lpo), lo = 1.0 - cfg.eps_clip, hi = 1.0 + cfg.eps_clip;
            const double s1 = r * A, s2 = fmin(fmax(r, lo), hi) * A;
            const double g2 = (r >= lo && r <= hi) ? A : 0.0;   // clamp's backward: the closed interval
            double g_r;
            if (s1 < s2) { obj = s1; g_r = A; }
            else if (s2 < s1) { obj = s2; g_r = g2; }
            else { obj = s1; g_r = 0.5 * A + 0.5 * g2; }
            if (cfg.dual_clip > 0.0 && A < 0.0) {   // ppo.py:190-194: max(min(s1, s2), c A) where A < 0
                const double cA = cfg.dual_clip * A;
                if (cA > obj) { obj = cA; g_r = 0.0; }
                else if (cA == obj) g_r *= 0.5;
            }
            g_logp = g_r * r;
        }
        const double gl = -g_logp * invM;
        if (in) {
            d_mu[b * ld_d + k] = (float)(gl * (z / o.sigma) * o.dmu);
            const double dc = o.pass * (gl * (z * z - 1.0) - cfg.ent_coef * invM);
            if (cond) d_sigma[b * ld_d + k] = (float)dc;
            else acc_col += dc;   // this lane's rows in row order
        }
        acc_obj += obj;
        acc_ent += ent;
    }
    // the workgroup's sums: the first lane of every group holds the group's; thread t < 2 adds the groups in order
    if (k == 0) { s_red[0][grp] = acc_obj; s_red[1][grp] = acc_ent; }
    if (!cond) s_col[grp * G + k] = acc_col;
    __syncthreads();
    const int t = threadIdx.x;
    if (t < 2) {
        double acc = 0.0;
        for (int q = 0; q < kGThreads / G; ++q) acc += s_red[t][q];
        partial[(int64_t)blockIdx.x * 4 + 2 * t] = acc;       // {clip_obj, 0, ent, 0}: tsm_ppo_finalize_many's layout
        partial[(int64_t)blockIdx.x * 4 + 2 * t + 1] = 0.0;
    }
    if (!cond && t < Ad) {   // d loss / d sigma_param of the workgroup's rows: component t over the groups in order
        double acc = 0.0;
        for (int q = 0; q < kGThreads / G; ++q) acc += s_col[q * G + t];
        col_partial[(int64_t)blockIdx.x * Ad + t] = acc;
    }
}

// slab 0's sigma columns <- the workgroups' rows of col_partial summed in block order; the other slabs' <- 0
__global__ __launch_bounds__(kWave) void gauss_sigma_fold_kernel(const double *__restrict__ col_partial, int32_t n_blocks,
                                                                 int32_t Ad, int32_t n_slab, float *__restrict__ out,
                                                                 int64_t slab_stride) {
    const int k = threadIdx.x;
    if (k >= Ad) return;
    double acc = 0.0;
    for (int b = 0; b < n_blocks; ++b) acc += col_partial[(int64_t)b * Ad + k];
    out[k] = (float)acc;
    for (int s = 1; s < n_slab; ++s) out[(int64_t)s * slab_stride + k] = 0.f;
}

int gauss_check(const char *who, int32_t Ad) {
    TSM_REQUIRE(Ad >= 1 && Ad <= TSM_CAC_MAX_ACT_DIM, "%s: act_dim = %d outside [1, %d]", who, Ad, TSM_CAC_MAX_ACT_DIM);
    return TSM_OK;
}

// B rows of Ad components: every element index stays below 2^31; pitches as tsm_sac_action's
int gauss_check_rows(const char *who, int64_t B, int32_t Ad, int64_t ld_mu, int64_t ld_sigma) {
    if (int rc = gauss_check(who, Ad)) return rc;
    if (int rc = tsm_q_check_rows(who, B)) return rc;
    TSM_REQUIRE(ld_mu >= Ad && (ld_sigma == 0 || ld_sigma >= Ad) && ld_mu <= (1 << 20) && ld_sigma <= (1 << 20),
                "%s: row pitches (%lld, %lld) for act_dim = %d (sigma: 0 = one row for all)", who, (long long)ld_mu,
                (long long)ld_sigma, Ad);
    return TSM_OK;
}

inline dim3 gauss_grid(int64_t B) { return dim3((unsigned)ceil_div(B, TSM_GAUSS_ROWS_PER_BLOCK)); }

// the kernel instance for act_dim: G = 8, 16, 32 or 64
#define GAUSS_BY_GROUP(Ad, KERNEL, ...)                                                                   \
    do {                                                                                                  \
        if ((Ad) <= 8) hipLaunchKernelGGL(KERNEL<8>, __VA_ARGS__);                                        \
        else if ((Ad) <= 16) hipLaunchKernelGGL(KERNEL<16>, __VA_ARGS__);                                 \
        else if ((Ad) <= 32) hipLaunchKernelGGL(KERNEL<32>, __VA_ARGS__);                                 \
        else hipLaunchKernelGGL(KERNEL<64>, __VA_ARGS__);                                                 \
    } while (0)
}  // namespace

TSM_EXPORT int tsm_gauss_check(int32_t act_dim) { return gauss_check("tsm_gauss_check", act_dim); }

TSM_EXPORT int tsm_gauss_sample(const float *mu_raw, int64_t ld_mu, const float *sigma_raw, int64_t ld_sigma, int64_t B,
                                int32_t act_dim, double max_action, int32_t unbounded, uint64_t seed, uint64_t offset,
                                const uint64_t *offset_dev, int32_t deterministic, int32_t bound_method, const float *low,
                                const float *high, float *act_out, float *logp_out, float *env_act_out, void *stream) {
    if (int rc = gauss_check_rows("tsm_gauss_sample", B, act_dim, ld_mu, ld_sigma)) return rc;
    TSM_REQUIRE(mu_raw && sigma_raw && act_out, "tsm_gauss_sample: null pointer");
    TSM_REQUIRE(bound_method >= 0 && bound_method <= 2, "tsm_gauss_sample: bound_method must be 0 (none), 1 (clip) or 2 (tanh)");
    TSM_REQUIRE((low == nullptr) == (high == nullptr), "tsm_gauss_sample: low and high come together");
    GAUSS_BY_GROUP(act_dim, gauss_sample_kernel, gauss_grid(B), dim3(kGThreads), 0, tsm_stream(stream), mu_raw, ld_mu,
                   sigma_raw, ld_sigma, B, act_dim, (float)max_action, unbounded, seed, offset, offset_dev, deterministic,
                   bound_method, low, high, act_out, logp_out, env_act_out);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_gauss_logp_entropy(const float *mu_raw, int64_t ld_mu, const float *sigma_raw, int64_t ld_sigma,
                                      const float *act, const int64_t *perm, int64_t B, int32_t act_dim, double max_action,
                                      int32_t unbounded, float *logp_out, float *entropy_out, void *stream) {
    if (int rc = gauss_check_rows("tsm_gauss_logp_entropy", B, act_dim, ld_mu, ld_sigma)) return rc;
    TSM_REQUIRE(mu_raw && sigma_raw && act && logp_out, "tsm_gauss_logp_entropy: null pointer");
    GAUSS_BY_GROUP(act_dim, gauss_logp_entropy_kernel, gauss_grid(B), dim3(kGThreads), 0, tsm_stream(stream), mu_raw, ld_mu,
                   sigma_raw, ld_sigma, act, perm, B, act_dim, (float)max_action, unbounded, logp_out, entropy_out);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_gauss_ppo_head(const float *mu_raw, int64_t ld_mu, const float *sigma_raw, int64_t ld_sigma,
                                  const float *act, const float *logp_old, const float *adv, const int64_t *perm,
                                  int64_t first_row, int64_t M, int32_t act_dim, const float *adv_stats,
                                  const tsm_ppo_cfg *cfg_host, double max_action, int32_t unbounded, float *d_mu_out,
                                  float *d_sigma_out, int64_t ld_d, double *partial_out, double *col_partial_out,
                                  void *stream) {
    if (int rc = gauss_check_rows("tsm_gauss_ppo_head", M, act_dim, ld_mu, ld_sigma)) return rc;
    TSM_REQUIRE(cfg_host, "tsm_gauss_ppo_head: null cfg");
    TSM_REQUIRE(cfg_host->loss_kind == 0 || cfg_host->loss_kind == 1, "tsm_gauss_ppo_head: loss_kind must be 0 or 1");
    TSM_REQUIRE(mu_raw && sigma_raw && act && adv && d_mu_out && partial_out && (cfg_host->loss_kind == 1 || logp_old),
                "tsm_gauss_ppo_head: null pointer");
    TSM_REQUIRE(ld_sigma == 0 ? col_partial_out != nullptr : d_sigma_out != nullptr,
                "tsm_gauss_ppo_head: a conditioned sigma needs d_sigma_out, a state-independent one col_partial_out");
    TSM_REQUIRE(ld_d >= act_dim && ld_d <= (1 << 20), "tsm_gauss_ppo_head: gradient row pitch %lld for act_dim = %d",
                (long long)ld_d, act_dim);
    TSM_REQUIRE(!cfg_host->adv_norm || adv_stats, "tsm_gauss_ppo_head: adv_norm needs adv_stats");
    TSM_REQUIRE(cfg_host->dual_clip <= 0.0 || cfg_host->dual_clip > 1.0,
                "Dual-clip PPO parameter should greater than 1.0 but got %g", cfg_host->dual_clip);  // ppo.py:124-126
    TSM_REQUIRE(first_row >= 0, "tsm_gauss_ppo_head: negative first_row");
    GaussCfg cfg;
    cfg.eps_clip = cfg_host->eps_clip;
    cfg.dual_clip = cfg_host->dual_clip;
    cfg.ent_coef = cfg_host->ent_coef;
    cfg.adv_norm = cfg_host->adv_norm;
    cfg.kind = cfg_host->loss_kind;
    GAUSS_BY_GROUP(act_dim, gauss_ppo_head_kernel, gauss_grid(M), dim3(kGThreads), 0, tsm_stream(stream), mu_raw, ld_mu,
                   sigma_raw, ld_sigma, act, logp_old, adv, perm, first_row, M, act_dim, adv_stats, cfg, (float)max_action,
                   unbounded, d_mu_out, d_sigma_out, ld_d, partial_out, col_partial_out);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_gauss_sigma_fold(const double *col_partial, int32_t n_blocks, int32_t act_dim, int32_t n_slab,
                                    float *slabs_out, int64_t slab_stride, void *stream) {
    if (int rc = gauss_check("tsm_gauss_sigma_fold", act_dim)) return rc;
    TSM_REQUIRE(n_blocks >= 1, "tsm_gauss_sigma_fold: n_blocks = %d", n_blocks);
    TSM_REQUIRE(n_slab >= 1 && (n_slab == 1 || slab_stride >= act_dim),
                "tsm_gauss_sigma_fold: n_slab = %d below 1 or slab pitch %lld below act_dim = %d", n_slab,
                (long long)slab_stride, act_dim);
    TSM_REQUIRE(col_partial && slabs_out, "tsm_gauss_sigma_fold: null pointer");
    hipLaunchKernelGGL(gauss_sigma_fold_kernel, dim3(1), dim3(kWave), 0, tsm_stream(stream), col_partial, n_blocks, act_dim,
                       n_slab, slabs_out, slab_stride);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}
