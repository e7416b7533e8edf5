// icm.hip -- Intrinsic Curiosity Module: the forward model's input rows, the row-wise head with its three gradients, and the
// join of the gradients that reach the feature net.
//
// Replaces the arithmetic of IntrinsicCuriosityModule.forward (/root/reference/tianshou/utils/net/discrete.py:411-429) between
// its three networks, `batch.rew += mse_loss * reward_scale` of _ICMMixin._icm_preprocess_batch
// (tianshou/algorithm/modelbased/icm.py:77-83) and the loss of _icm_update with its backward down to the networks' outputs
// (icm.py:95-101).  The feature net, the forward model and the inverse model run in csrc/dense.hip.
//
// Row layout: the feature net runs once over 2R interleaved rows, obs of row r at 2r and obs_next at 2r + 1, so
// phi [2R][F] viewed as [R][2F] is [phi1 | phi2], the inverse model's input.
//
// Head: one wave per row, kRowsPerWave rows after one another, 4 waves per workgroup (the shape of csrc/dsac.hip).  Lane l
// holds feature columns l, l + 64, ... and action l (n_act <= 64).  A row sum is formed in f64 from the f32 inputs: every
// lane adds its columns in index order, then the xor butterfly wave_sum; a per-workgroup sum is lane 0's f64 running sum over
// the wave's rows followed by the four waves in order.  So two runs give the same bits.
//
// Per row r, with d[k] = phi2_hat[r][k] - phi2[r][k], x = act_hat[r], a = act[r], w = forward_loss_weight, s = lr_scale:
//   mse = 0.5 sum_k d[k]^2                       (0.5 * F.mse_loss(reduction="none").sum(1))
//   ce  = logsumexp(x) - x[a]                    (F.cross_entropy)
//   loss = ((1 - w) mean_r ce + w mean_r mse) s
//   d loss / d phi2_hat[r][k] = s w d[k] / R     d loss / d phi2[r][k] = -s w d[k] / R   (nothing is detached)
//   d loss / d act_hat[r][j]  = s (1 - w) (softmax(x)[j] - 1[j = a]) / R
// each formed in f64 and rounded to f32 once.  An action outside [0, n_act) reads nothing: the row's mse and ce are NaN (so
// is what it adds to its reward) and its three gradient rows are zero, as in tsm_dsac_critic_head.
#include "common.h"
#include "q_head_dev.h"

namespace {
constexpr int kIThreads = 256;
constexpr int kIWaves = kIThreads / kWave;
constexpr int kIRowsPerWave = TSM_ICM_ROWS_PER_BLOCK / kIWaves;
constexpr int kIMaxF = 512;
static_assert(kQHeadMaxA <= kWave, "one lane per action");
static_assert(kIRowsPerWave * kIWaves == TSM_ICM_ROWS_PER_BLOCK, "rows per workgroup");

__global__ __launch_bounds__(kIThreads) void icm_rows_kernel(const float *__restrict__ phi, const int64_t *__restrict__ act,
                                                             int64_t R, int32_t F, int32_t A, float *__restrict__ x_fwd) {
    const int64_t W = (int64_t)F + A, n = R * W;
    for (int64_t e = (int64_t)blockIdx.x * kIThreads + threadIdx.x; e < n; e += (int64_t)gridDim.x * kIThreads) {
        const int64_t r = e / W;
        const int c = (int)(e - r * W);
        // phi1 of row r is row 2r of phi; an action outside [0, A) matches no column: an all-zero one-hot
        x_fwd[e] = c < F ? phi[2 * r * F + c] : (act[r] == (int64_t)(c - F) ? 1.f : 0.f);
    }
}

__global__ __launch_bounds__(kIThreads) void icm_head_kernel(const float *__restrict__ phi2_hat, const float *__restrict__ phi2,
                                                             int64_t phi2_stride, const float *__restrict__ act_hat,
                                                             const int64_t *__restrict__ act, float *__restrict__ rew_io,
                                                             const int64_t *__restrict__ ids, int64_t R, int32_t F, int32_t A,
                                                             float reward_scale, double w_fwd, double lr_scale,
                                                             float *__restrict__ mse_out, float *__restrict__ d_phi2_hat,
                                                             float *__restrict__ d_phi2_fwd, float *__restrict__ d_act_hat,
                                                             double *__restrict__ partial) {
    __shared__ double s_red[2][kIWaves];
    const int t = threadIdx.x, lane = t & (kWave - 1), w = t / kWave;
    const double g_f = lr_scale * w_fwd / (double)R, g_i = lr_scale * (1.0 - w_fwd) / (double)R;
    double acc_f = 0.0, acc_i = 0.0;
    for (int rr = 0; rr < kIRowsPerWave; ++rr) {
        const int64_t r = (int64_t)blockIdx.x * TSM_ICM_ROWS_PER_BLOCK + w * kIRowsPerWave + rr;
        if (r >= R) break;
        const int64_t ac = act[r];
        const bool ok = ac >= 0 && ac < A;   // an action outside [0, A) reads nothing and poisons the losses
        const double nanv = (double)__builtin_nanf("");
        // forward model: mse and the two gradients it sends into phi2_hat and phi2
        const float *ph = phi2_hat + r * F, *p2 = phi2 + r * phi2_stride;
        double sq = 0.0;
        for (int k = lane; k < F; k += kWave) {
            const double d = (double)ph[k] - (double)p2[k];
            sq += d * d;
            const float g = ok ? (float)(g_f * d) : 0.f;
            d_phi2_hat[r * F + k] = g;
            d_phi2_fwd[r * F + k] = -g;
        }
        const double mse = ok ? 0.5 * wave_sum(sq) : nanv;
        // inverse model: cross entropy of act_hat against act, its softmax gradient
        const bool in = lane < A;
        const float x = in ? act_hat[r * A + lane] : -INFINITY;
        const float mx = wave_max(x);
        const double tl = in ? (double)x - (double)mx : 0.0;
        const double e = in ? exp(tl) : 0.0;
        const double s = wave_sum(e);
        const double xa = wave_sum(ok && lane == (int)ac ? tl : 0.0);
        const double ce = ok ? log(s) - xa : nanv;
        if (in) d_act_hat[r * A + lane] = ok ? (float)(g_i * (e / s - (lane == (int)ac ? 1.0 : 0.0))) : 0.f;
        if (lane == 0) {
            const float m32 = (float)mse;
            mse_out[r] = m32;
            if (rew_io) {
                const int64_t i = ids ? ids[r] : r;
                rew_io[i] = rew_io[i] + m32 * reward_scale;   // an f32 product and an f32 add (no contraction: -ffp-contract=off)
            }
            acc_f += mse;
            acc_i += ce;
        }
    }
    tsm_store_partials(acc_f, acc_i, t, lane, w, s_red, partial);
}

__global__ __launch_bounds__(kIThreads) void icm_join_grad_kernel(const float *__restrict__ g_fwd, const float *g_inv,
                                                                  const float *__restrict__ d_phi2_fwd, int64_t R, int32_t F,
                                                                  float *d_out) {
    const int64_t n = R * F;
    for (int64_t e = (int64_t)blockIdx.x * kIThreads + threadIdx.x; e < n; e += (int64_t)gridDim.x * kIThreads) {
        const int64_t r = e / F;
        const int k = (int)(e - r * F);
        const int64_t o1 = 2 * r * F + k, o2 = o1 + F;   // g_inv [R][2F] and d_out [2R][F] share this layout (and may alias)
        const float a = g_fwd[e] + g_inv[o1];
        const float b = g_inv[o2] + d_phi2_fwd[e];
        d_out[o1] = a;
        d_out[o2] = b;
    }
}

int icm_check(const char *who, int32_t F, int32_t A) {
    TSM_REQUIRE(F >= 1 && F <= kIMaxF, "%s: feature_dim = %d outside [1, %d]", who, F, kIMaxF);
    return tsm_q_check_act(who, A);
}

// R * (2 feature_dim + n_act) stays below 2^31
int icm_check_rows(const char *who, int64_t R, int32_t F, int32_t A) {
    if (int rc = icm_check(who, F, A)) return rc;
    const int64_t r_max = (((int64_t)1 << 31) - 1) / (2 * (int64_t)F + A);
    TSM_REQUIRE(R >= 1 && R <= r_max, "%s: R = %lld outside [1, %lld]: R (2 feature_dim + n_act) stays below 2^31", who,
                (long long)R, (long long)r_max);
    return TSM_OK;
}

inline dim3 icm_flat_grid(int64_t n) { return dim3((unsigned)(ceil_div(n, kIThreads) < 4096 ? ceil_div(n, kIThreads) : 4096)); }
}  // namespace

TSM_EXPORT int tsm_icm_check(int32_t feature_dim, int32_t n_act) { return icm_check("tsm_icm_check", feature_dim, n_act); }

TSM_EXPORT int tsm_icm_rows(const float *phi, const int64_t *act, int64_t R, int32_t feature_dim, int32_t n_act, float *x_fwd,
                            void *stream) {
    if (int rc = icm_check_rows("tsm_icm_rows", R, feature_dim, n_act)) return rc;
    TSM_REQUIRE(phi && act && x_fwd, "tsm_icm_rows: null pointer");
    hipLaunchKernelGGL(icm_rows_kernel, icm_flat_grid(R * ((int64_t)feature_dim + n_act)), dim3(kIThreads), 0, tsm_stream(stream),
                       phi, act, R, feature_dim, n_act, x_fwd);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_icm_head(const float *phi2_hat, const float *phi2, int64_t phi2_row_stride, const float *act_hat,
                            const int64_t *act, float *rew_io, const int64_t *ids, int64_t R, int32_t feature_dim, int32_t n_act,
                            double reward_scale, double forward_loss_weight, double lr_scale, float *mse, float *d_phi2_hat,
                            float *d_phi2_fwd, float *d_act_hat, double *partial, void *stream) {
    if (int rc = icm_check_rows("tsm_icm_head", R, feature_dim, n_act)) return rc;
    TSM_REQUIRE(phi2_row_stride >= feature_dim, "tsm_icm_head: phi2 row stride %lld < feature_dim %d", (long long)phi2_row_stride,
                feature_dim);
    TSM_REQUIRE(phi2_hat && phi2 && act_hat && act && mse && d_phi2_hat && d_phi2_fwd && d_act_hat && partial,
                "tsm_icm_head: null pointer");
    TSM_REQUIRE(rew_io || !ids, "tsm_icm_head: ids without rew_io");
    hipLaunchKernelGGL(icm_head_kernel, dim3((unsigned)ceil_div(R, TSM_ICM_ROWS_PER_BLOCK)), dim3(kIThreads), 0, tsm_stream(stream),
                       phi2_hat, phi2, phi2_row_stride, act_hat, act, rew_io, ids, R, feature_dim, n_act, (float)reward_scale,
                       forward_loss_weight, lr_scale, mse, d_phi2_hat, d_phi2_fwd, d_act_hat, partial);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_icm_join_grad(const float *g_fwd, const float *g_inv, const float *d_phi2_fwd, int64_t R, int32_t feature_dim,
                                 float *d_out, void *stream) {
    if (int rc = icm_check_rows("tsm_icm_join_grad", R, feature_dim, 1)) return rc;
    TSM_REQUIRE(g_fwd && g_inv && d_phi2_fwd && d_out, "tsm_icm_join_grad: null pointer");
    hipLaunchKernelGGL(icm_join_grad_kernel, icm_flat_grid(R * (int64_t)feature_dim), dim3(kIThreads), 0, tsm_stream(stream), g_fwd,
                       g_inv, d_phi2_fwd, R, feature_dim, d_out);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}
