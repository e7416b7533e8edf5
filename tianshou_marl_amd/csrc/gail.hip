// gail.hip -- GAIL: the expert draw, the discriminator's input rows, the discriminator reward, the row-wise head of the
// discriminator loss with its gradient, and the step's three statistics.
//
// Replaces, of tianshou/algorithm/imitation/gail.py: `expert_buffer.sample(bsz)` (:227), `torch.cat([obs, act], dim=1)` of
// `disc` (:208-212, on one-hot actions), `batch.rew = -F.logsigmoid(-disc(batch))` (:204-205) and the loss of
// _update_with_batch with its backward down to the logits and its two accuracies (:226-235).  The discriminator itself runs in
// csrc/dense.hip.
//
// A pair is one (buffer row, agent) sample: id p indexes obs_store as [S B N][D], act_store as i32 [S B N] and rew_store as
// [S B N], read in place.
//
// Head: one thread per row, TSM_GAIL_ROWS_PER_BLOCK rows per workgroup; the policy rows come first, then the expert rows, so a
// workgroup may hold both.  With l a logit:
//   loss = mean_pi softplus(l) + mean_exp softplus(-l)        (-logsigmoid(-l_pi).mean() - logsigmoid(l_exp).mean())
//   d loss / d l = sigmoid(l) / Rp (policy row), (sigmoid(l) - 1) / Re = -sigmoid(-l) / Re (expert row)
// each formed in f64 from the f32 logit and rounded to f32 once.  A workgroup's four sums are each wave's xor butterfly over its
// 64 rows followed by the four waves in order; tsm_gail_finalize adds the workgroups in index order.  So two runs give the same
// bits.
#include "common.h"
#include "philox.h"
#include "q_head_dev.h"

namespace {
constexpr int kGThreads = 256;
constexpr int kGWaves = kGThreads / kWave;
constexpr uint64_t kGailKey = 0x4741494C45585054ull;   // folded into the seed: a Philox key no other draw uses
static_assert(TSM_GAIL_ROWS_PER_BLOCK == kGThreads, "one thread per row");

__device__ __forceinline__ double gail_softplus(double x) { return fmax(x, 0.0) + log1p(exp(-fabs(x))); }

__device__ __forceinline__ double gail_sigmoid(double x) {
    const double e = exp(-fabs(x));
    return x >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
}

__global__ __launch_bounds__(kGThreads) void gail_draw_kernel(const int64_t *__restrict__ valid, uint64_t n_pairs, int32_t N,
                                                              int64_t R, uint64_t seed, uint64_t counter,
                                                              const uint64_t *__restrict__ counter_dev,
                                                              int64_t *__restrict__ ids_out) {
    const int64_t i = (int64_t)blockIdx.x * kGThreads + threadIdx.x;
    if (i >= R) return;
    uint32_t w[4];
    tsm_philox4(seed ^ kGailKey, counter + (counter_dev ? *counter_dev : 0ull) + (uint64_t)i, w);
    const uint64_t j = ((uint64_t)w[0] * n_pairs) >> 32;   // n_pairs < 2^32: the product fits 64 bits, j < n_pairs
    const int64_t row = (int64_t)(j / (uint64_t)N), a = (int64_t)(j % (uint64_t)N);
    ids_out[i] = (valid ? valid[row] : row) * N + a;
}

__global__ __launch_bounds__(kGThreads) void gail_rows_kernel(const float *__restrict__ obs, const int32_t *__restrict__ act,
                                                              const int64_t *__restrict__ ids, int64_t R, int32_t D, int32_t A,
                                                              float *__restrict__ x_out) {
    const int64_t W = (int64_t)D + A, n = R * W;
    for (int64_t e = (int64_t)blockIdx.x * kGThreads + threadIdx.x; e < n; e += (int64_t)gridDim.x * kGThreads) {
        const int64_t r = e / W;
        const int c = (int)(e - r * W);
        const int64_t p = ids ? ids[r] : r;
        // an action outside [0, A) matches no column: an all-zero one-hot
        x_out[e] = c < D ? obs[p * D + c] : (act[p] == c - D ? 1.f : 0.f);
    }
}

__global__ __launch_bounds__(kGThreads) void gail_reward_kernel(const float *__restrict__ logits, const int64_t *__restrict__ ids,
                                                                int64_t R, float *__restrict__ rew_io) {
    const int64_t r = (int64_t)blockIdx.x * kGThreads + threadIdx.x;
    if (r >= R) return;
    rew_io[ids ? ids[r] : r] = (float)gail_softplus((double)logits[r]);
}

__global__ __launch_bounds__(kGThreads) void gail_head_kernel(const float *__restrict__ logits, int64_t Rp, int64_t Re,
                                                              float *__restrict__ d_logits, double *__restrict__ partial) {
    __shared__ double s_red[4][kGWaves];
    const int t = threadIdx.x, lane = t & (kWave - 1), w = t / kWave;
    const int64_t r = (int64_t)blockIdx.x * TSM_GAIL_ROWS_PER_BLOCK + t;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    if (r < Rp + Re) {
        const double l = (double)logits[r];
        if (r < Rp) {
            v[0] = gail_softplus(l);
            v[2] = l < 0.0 ? 1.0 : 0.0;
            d_logits[r] = (float)(gail_sigmoid(l) / (double)Rp);
        } else {
            v[1] = gail_softplus(-l);
            v[3] = l > 0.0 ? 1.0 : 0.0;
            d_logits[r] = (float)(-gail_sigmoid(-l) / (double)Re);   // sigmoid(l) - 1, without the cancellation
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double s = wave_sum(v[k]);
        if (lane == 0) s_red[k][w] = s;
    }
    __syncthreads();
    if (t < 4) {
        double acc = 0.0;
        for (int k = 0; k < kGWaves; ++k) acc += s_red[t][k];
        partial[(int64_t)blockIdx.x * 4 + t] = acc;
    }
}

__global__ __launch_bounds__(kWave) void gail_finalize_kernel(const double *__restrict__ partial, int64_t nb, int64_t Rp,
                                                              int64_t Re, float *__restrict__ out) {
    if (threadIdx.x != 0) return;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t b = 0; b < nb; ++b)   // the workgroups in index order
        for (int k = 0; k < 4; ++k) s[k] += partial[4 * b + k];
    out[0] = (float)(s[0] / (double)Rp + s[1] / (double)Re);
    out[1] = (float)(s[2] / (double)Rp);
    out[2] = (float)(s[3] / (double)Re);
}

int gail_check(const char *who, int32_t D, int32_t A) {
    TSM_REQUIRE(D >= 1, "%s: obs_dim = %d below 1", who, D);
    return tsm_q_check_act(who, A);
}

// R * (obs_dim + n_act) stays below 2^31
int gail_check_rows(const char *who, int64_t R, int32_t D, int32_t A) {
    if (int rc = gail_check(who, D, A)) return rc;
    const int64_t r_max = (((int64_t)1 << 31) - 1) / ((int64_t)D + A);
    TSM_REQUIRE(R >= 1 && R <= r_max, "%s: R = %lld outside [1, %lld]: R (obs_dim + n_act) stays below 2^31", who, (long long)R,
                (long long)r_max);
    return TSM_OK;
}

// a per-row launch: R rows of one value each (obs_dim + n_act = 1 in the bound above)
int gail_check_count(const char *who, const char *what, int64_t R) {
    TSM_REQUIRE(R >= 1 && R < ((int64_t)1 << 31), "%s: %s = %lld outside [1, 2^31)", who, what, (long long)R);
    return TSM_OK;
}

inline dim3 gail_grid(int64_t n) { return dim3((unsigned)ceil_div(n, kGThreads)); }
}  // namespace

TSM_EXPORT int tsm_gail_check(int32_t obs_dim, int32_t n_act) { return gail_check("tsm_gail_check", obs_dim, n_act); }

TSM_EXPORT int tsm_gail_draw(const int64_t *valid, int64_t n_valid, int32_t n_agent, int64_t R, uint64_t seed, uint64_t counter,
                             const uint64_t *counter_dev, int64_t *ids_out, void *stream) {
    TSM_REQUIRE(n_agent >= 1 && n_valid >= 1 && n_valid <= (((int64_t)1 << 32) - 1) / n_agent,
                "tsm_gail_draw: n_valid n_agent = %lld x %d outside [1, 2^32)", (long long)n_valid, n_agent);
    if (int rc = gail_check_count("tsm_gail_draw", "R", R)) return rc;
    TSM_REQUIRE(ids_out, "tsm_gail_draw: null pointer");
    hipLaunchKernelGGL(gail_draw_kernel, gail_grid(R), dim3(kGThreads), 0, tsm_stream(stream), valid,
                       (uint64_t)n_valid * (uint64_t)n_agent, n_agent, R, seed, counter, counter_dev, ids_out);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_gail_rows(const float *obs, const int32_t *act, const int64_t *ids, int64_t R, int32_t obs_dim, int32_t n_act,
                             float *x_out, void *stream) {
    if (int rc = gail_check_rows("tsm_gail_rows", R, obs_dim, n_act)) return rc;
    TSM_REQUIRE(obs && act && x_out, "tsm_gail_rows: null pointer");
    const int64_t nb = ceil_div(R * ((int64_t)obs_dim + n_act), kGThreads);
    hipLaunchKernelGGL(gail_rows_kernel, dim3((unsigned)(nb < 4096 ? nb : 4096)), dim3(kGThreads), 0, tsm_stream(stream), obs, act,
                       ids, R, obs_dim, n_act, x_out);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_gail_reward(const float *logits, const int64_t *ids, int64_t R, float *rew_io, void *stream) {
    if (int rc = gail_check_count("tsm_gail_reward", "R", R)) return rc;
    TSM_REQUIRE(logits && rew_io, "tsm_gail_reward: null pointer");
    hipLaunchKernelGGL(gail_reward_kernel, gail_grid(R), dim3(kGThreads), 0, tsm_stream(stream), logits, ids, R, rew_io);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_gail_head(const float *logits, int64_t Rp, int64_t Re, float *d_logits, double *partial, void *stream) {
    TSM_REQUIRE(Rp >= 1 && Re >= 1, "tsm_gail_head: Rp = %lld, Re = %lld: each at least 1", (long long)Rp, (long long)Re);
    if (int rc = gail_check_count("tsm_gail_head", "Rp + Re", Rp + Re)) return rc;
    TSM_REQUIRE(logits && d_logits && partial, "tsm_gail_head: null pointer");
    hipLaunchKernelGGL(gail_head_kernel, dim3((unsigned)ceil_div(Rp + Re, TSM_GAIL_ROWS_PER_BLOCK)), dim3(kGThreads), 0,
                       tsm_stream(stream), logits, Rp, Re, d_logits, partial);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_gail_finalize(const double *partial, int64_t n_blocks, int64_t Rp, int64_t Re, float *out, void *stream) {
    TSM_REQUIRE(n_blocks >= 1 && Rp >= 1 && Re >= 1, "tsm_gail_finalize: n_blocks = %lld, Rp = %lld, Re = %lld: each at least 1",
                (long long)n_blocks, (long long)Rp, (long long)Re);
    TSM_REQUIRE(partial && out, "tsm_gail_finalize: null pointer");
    hipLaunchKernelGGL(gail_finalize_kernel, dim3(1), dim3(kWave), 0, tsm_stream(stream), partial, n_blocks, Rp, Re, out);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}
