// bcq.hip -- BCQ (arXiv:1812.02900): what its update and its acting add to csrc/cac.hip.
//
// Replaces, in tianshou:
//   VAE.forward's clamp, exp, reparameterised latent and torch.cat([state, z])                 utils/net/continuous.py:487-495
//   repeat_interleave, decode's clamped normals and its torch.cat                              imitation/bcq.py:213, continuous.py:508-510
//   max_action * tanh(decoder(.)) and the torch.cat([obs, act]) that follows it                continuous.py:513
//   the lmbda-weighted min / max of the lagged critics, the max over the samples, the target   bcq.py:223-237
//   recon_loss, KL_loss and vae_loss.backward() down to the decoder's raw output               bcq.py:203-208
//     and from the decoder's input gradient to the encoder head's output
//   Perturbation.forward behind its net, and its backward                                      continuous.py:429-432
//   q1.argmax(0) and act[max_indice] per observation                                           bcq.py:103-115
// The encoder, the decoder, the perturbation net and the critics run in csrc/dense.hip; the normals are tsm_cac_normal's, the
// critics' mse head tsm_cac_critic_head, the actor's loss head tsm_cac_det_actor_head fed tsm_bcq_perturb's factor.
//
// With head = [mean | ls] the encoder's output, c = clamp(ls, -4, 15), std = exp(c), z = mean + std eps, recon = M tanh(raw):
//   vae_loss = mean_{b,k} (act - recon)^2 + (1 / 2) mean_{b,j} (-c + (std^2 + mean^2 - 1) / 2)       (-log std = -c)
//   d vae_loss / d raw[b][k]  = 2 (recon - act) / (B Ad) M (1 - tanh^2)
//   d vae_loss / d mean[b][j] = dz + mean / (2 B L),   dz the decoder's input gradient at column D + j
//   d vae_loss / d ls[b][j]   = pass (dz eps std + (std^2 - 1) / (2 B L)),  pass = 1[-4 <= ls <= 15] (torch.clamp's backward)
// All arithmetic is float64 from the float32 inputs, rounded once; nothing but the inputs is saved between the forward and the
// backward (std, the clamp and tanh are formed again from them: the same float64 numbers).  The row writers are one float per
// thread and step: no alignment is asked of a row.  Sums: the xor butterfly per wave, lane 0's running sum over the wave's rows,
// the four waves in order, tsm_qmix_finalize over the workgroups: two runs give the same bits.
#include "common.h"
#include "q_head_dev.h"

namespace {
constexpr int kBThreads = 256;
constexpr int kBWaves = kBThreads / kWave;
constexpr int kBRowsPerWave = TSM_CAC_ROWS_PER_BLOCK / kBWaves;
constexpr int kMaxLatent = 2 * TSM_CAC_MAX_ACT_DIM;
constexpr double kLsMin = -4.0, kLsMax = 15.0;   // continuous.py:489
constexpr float kZClip = 0.5f;                   // continuous.py:509
static_assert(TSM_CAC_MAX_ACT_DIM <= kWave && kMaxLatent <= 2 * kWave, "a lane holds one action and two latent components");

#define BCQ_ELEMENT_LOOP(e, n)                                                                                 \
    for (int64_t e = (int64_t)blockIdx.x * kBThreads + threadIdx.x; e < (n); e += (int64_t)gridDim.x * kBThreads)

__device__ __forceinline__ double bcq_std(float ls) { return exp(fmin(fmax((double)ls, kLsMin), kLsMax)); }

__global__ __launch_bounds__(kBThreads) void bcq_latent_kernel(const float *__restrict__ head, const float *__restrict__ eps,
                                                               const float *__restrict__ obs, int64_t B, int32_t D, int32_t L,
                                                               float *__restrict__ x_dec, float *__restrict__ std_out) {
    const int64_t W = (int64_t)D + L;
    BCQ_ELEMENT_LOOP(e, B * W) {
        const int64_t r = e / W;
        const int c = (int)(e - r * W);
        if (c < D) {
            x_dec[e] = obs[r * D + c];
        } else {
            const int j = c - D;
            const double sd = bcq_std(head[r * 2 * L + L + j]);
            std_out[r * L + j] = (float)sd;
            x_dec[e] = (float)((double)head[r * 2 * L + j] + sd * (double)eps[r * L + j]);
        }
    }
}

__global__ __launch_bounds__(kBThreads) void bcq_decode_rows_kernel(const float *__restrict__ src_a, int64_t n_a, int64_t rep_a,
                                                                    const float *__restrict__ src_b, int64_t n_b,
                                                                    const float *__restrict__ z, int32_t D, int32_t L,
                                                                    float *__restrict__ out) {
    const int64_t W = (int64_t)D + L, na = n_a * rep_a;
    BCQ_ELEMENT_LOOP(e, (na + n_b) * W) {
        const int64_t r = e / W;
        const int c = (int)(e - r * W);
        if (c < D) {
            out[e] = r < na ? src_a[(r / rep_a) * D + c] : src_b[(r - na) * D + c];
        } else {
            const float v = z[r * L + (c - D)];
            out[e] = v != v ? v : fminf(fmaxf(v, -kZClip), kZClip);   // torch.clamp keeps a NaN
        }
    }
}

__global__ __launch_bounds__(kBThreads) void bcq_action_rows_kernel(const float *__restrict__ raw, const float *__restrict__ x_dec,
                                                                    int64_t n, int32_t D, int32_t L, int32_t Ad, double M,
                                                                    float *__restrict__ x) {
    const int64_t W = (int64_t)D + Ad, Wd = (int64_t)D + L;
    BCQ_ELEMENT_LOOP(e, n * W) {
        const int64_t r = e / W;
        const int c = (int)(e - r * W);
        x[e] = c < D ? x_dec[r * Wd + c] : (float)(M * tanh((double)raw[r * Ad + (c - D)]));
    }
}

// One thread per transition: its K samples in order; a NaN is kept, as torch.max keeps it.
__global__ __launch_bounds__(kBThreads) void bcq_target_kernel(const float *__restrict__ q1, const float *__restrict__ q2,
                                                               const float *__restrict__ rew, const uint8_t *__restrict__ vmask,
                                                               int64_t B, int64_t K, double gamma, double lmbda,
                                                               float *__restrict__ target) {
    const int64_t b = (int64_t)blockIdx.x * kBThreads + threadIdx.x;
    if (b >= B) return;
    double best = 0.0;
    for (int64_t k = 0; k < K; ++k) {
        const double a = (double)q1[b * K + k], c = (double)q2[b * K + k];
        const double lo = (a != a || c != c) ? a + c : fmin(a, c), hi = (a != a || c != c) ? a + c : fmax(a, c);
        const double v = lmbda * lo + (1.0 - lmbda) * hi;
        if (k == 0 || v > best || (v != v && best == best)) best = v;
    }
    target[b] = (float)((double)rew[b] + (vmask[b] ? 1.0 : 0.0) * gamma * best);
}

// One wave per row: lane k the action component k, lanes j and j + 64 the latent components.
// partial {sum_b (sum_k (act - recon)^2 / Ad + sum_j kl / (2 L)), sum_b sum_j kl / L}: tsm_qmix_finalize gives {vae_loss, KL_loss}.
__global__ __launch_bounds__(kBThreads) void bcq_vae_head_kernel(const float *__restrict__ raw, const float *__restrict__ act,
                                                                 const float *__restrict__ head, int64_t B, int32_t Ad, int32_t L,
                                                                 double M, float *__restrict__ d_raw,
                                                                 double *__restrict__ partial) {
    __shared__ double s_red[2][kBWaves];
    const int t = threadIdx.x, lane = t & (kWave - 1), w = t / kWave;
    double acc0 = 0.0, acc1 = 0.0;
    for (int rr = 0; rr < kBRowsPerWave; ++rr) {
        const int64_t b = (int64_t)blockIdx.x * TSM_CAC_ROWS_PER_BLOCK + w * kBRowsPerWave + rr;
        if (b >= B) continue;   // the whole wave leaves together
        double sq = 0.0, kl = 0.0;
        if (lane < Ad) {
            const double th = tanh((double)raw[b * Ad + lane]);
            const double diff = M * th - (double)act[b * Ad + lane];
            sq = diff * diff;
            d_raw[b * Ad + lane] = (float)(2.0 * diff / ((double)B * (double)Ad) * M * (1.0 - th * th));
        }
        for (int j = lane; j < L; j += kWave) {
            const double mean = (double)head[b * 2 * L + j], ls = (double)head[b * 2 * L + L + j];
            const double c = fmin(fmax(ls, kLsMin), kLsMax), sd = exp(c);
            kl += -c + (sd * sd + mean * mean - 1.0) / 2.0;
        }
        sq = wave_sum(sq);
        kl = wave_sum(kl);
        if (lane == 0) {
            acc0 += sq / (double)Ad + kl / (2.0 * (double)L);
            acc1 += kl / (double)L;
        }
    }
    tsm_store_partials(acc0, acc1, t, lane, w, s_red, partial);
}

__global__ __launch_bounds__(kBThreads) void bcq_latent_grad_kernel(const float *__restrict__ dz, const float *__restrict__ head,
                                                                    const float *__restrict__ eps, int64_t B, int32_t L,
                                                                    float *__restrict__ d_head) {
    const double inv = 1.0 / (2.0 * (double)B * (double)L);
    BCQ_ELEMENT_LOOP(e, B * L) {
        const int64_t r = e / L;
        const int j = (int)(e - r * L);
        const double mean = (double)head[r * 2 * L + j], ls = (double)head[r * 2 * L + L + j], g = (double)dz[e];
        const double sd = bcq_std((float)ls);
        const double pass = (ls >= kLsMin && ls <= kLsMax) ? 1.0 : 0.0;
        d_head[r * 2 * L + j] = (float)(g + mean * inv);
        d_head[r * 2 * L + L + j] = (float)(pass * (g * (double)eps[e] * sd + (sd * sd - 1.0) * inv));
    }
}

__global__ __launch_bounds__(kBThreads) void bcq_perturb_kernel(const float *__restrict__ raw_p, const float *__restrict__ x_in,
                                                                int64_t n, int32_t D, int32_t Ad, double phi, double M,
                                                                float *__restrict__ x_out, float *__restrict__ factor) {
    const int64_t W = (int64_t)D + Ad;
    BCQ_ELEMENT_LOOP(e, n * W) {
        const int64_t r = e / W;
        const int c = (int)(e - r * W);
        if (c < D) {
            x_out[e] = x_in[e];
        } else {
            const int k = c - D;
            const double th = tanh((double)raw_p[r * Ad + k]);
            const double u = (double)x_in[e] + phi * M * th;
            x_out[e] = (float)(u != u ? u : fmin(fmax(u, -M), M));
            if (factor) factor[r * Ad + k] = (float)((u >= -M && u <= M) ? phi * (1.0 - th * th) : 0.0);
        }
    }
}

// One wave per observation: lane l walks the candidates l, l + 64, ... in order, then the butterfly; of equal values the lower
// index wins, and a NaN counts as the maximum (torch.argmax).
__device__ __forceinline__ bool bcq_better(float v, int i, float bv, int bi) {
    const bool vn = v != v, bn = bv != bv;
    if (vn || bn) return vn && (!bn || i < bi);
    return v > bv || (v == bv && i < bi);
}

__global__ __launch_bounds__(kBThreads) void bcq_select_kernel(const float *__restrict__ q, const float *__restrict__ rows,
                                                               int64_t ld, int32_t col0, int64_t n, int32_t S, int32_t Ad,
                                                               float *__restrict__ act_out, int32_t *__restrict__ index) {
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    const int64_t g = (int64_t)blockIdx.x * kBWaves + w;
    if (g >= n) return;   // the whole wave leaves together
    float best = 0.f;
    int bi = 0x7fffffff;
    for (int s = lane; s < S; s += kWave) {
        const float v = q[g * S + s];
        if (bi == 0x7fffffff || bcq_better(v, s, best, bi)) { best = v; bi = s; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(best, off, kWave);
        const int oi = __shfl_xor(bi, off, kWave);
        if (oi != 0x7fffffff && (bi == 0x7fffffff || bcq_better(ov, oi, best, bi))) { best = ov; bi = oi; }
    }
    if (lane < Ad) act_out[g * Ad + lane] = rows[(g * S + bi) * ld + col0 + lane];
    if (lane == 0) index[g] = bi;
}

int bcq_check(const char *who, int32_t Ad, int32_t L, int32_t K) {
    TSM_REQUIRE(Ad >= 1 && Ad <= TSM_CAC_MAX_ACT_DIM, "%s: act_dim = %d outside [1, %d]", who, Ad, TSM_CAC_MAX_ACT_DIM);
    TSM_REQUIRE(L >= 1 && L <= kMaxLatent, "%s: latent_dim = %d outside [1, %d]", who, L, kMaxLatent);
    TSM_REQUIRE(K >= 1, "%s: the number of sampled actions should be at least 1 but got: %d", who, K);
    return TSM_OK;
}

// n rows of at most W floats: every element index stays below 2^31
int bcq_check_rows(const char *who, int64_t n, int64_t W) {
    TSM_REQUIRE(n >= 1 && W >= 1 && W <= (1 << 20) && n <= (((int64_t)1 << 31) - 1) / W,
                "%s: %lld rows of %lld floats: rows times width stays below 2^31", who, (long long)n, (long long)W);
    return TSM_OK;
}

inline dim3 bcq_grid(int64_t n_elem) {
    const int64_t nb = ceil_div(n_elem, kBThreads);
    return dim3((unsigned)(nb < 4096 ? nb : 4096));
}
}  // namespace

TSM_EXPORT int tsm_bcq_check(int32_t act_dim, int32_t latent_dim, int32_t num_sampled) {
    return bcq_check("tsm_bcq_check", act_dim, latent_dim, num_sampled);
}

TSM_EXPORT int tsm_bcq_latent(const float *head, const float *eps, const float *obs, int64_t B, int32_t obs_dim,
                              int32_t latent_dim, float *x_dec_out, float *std_out, void *stream) {
    if (int rc = bcq_check("tsm_bcq_latent", 1, latent_dim, 1)) return rc;
    TSM_REQUIRE(obs_dim >= 1, "tsm_bcq_latent: obs_dim = %d below 1", obs_dim);
    if (int rc = bcq_check_rows("tsm_bcq_latent", B, (int64_t)obs_dim + 2 * latent_dim)) return rc;
    TSM_REQUIRE(head && eps && obs && x_dec_out && std_out, "tsm_bcq_latent: null pointer");
    hipLaunchKernelGGL(bcq_latent_kernel, bcq_grid(B * ((int64_t)obs_dim + latent_dim)), dim3(kBThreads), 0, tsm_stream(stream),
                       head, eps, obs, B, obs_dim, latent_dim, x_dec_out, std_out);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_bcq_decode_rows(const float *src_a, int64_t n_a, int32_t rep_a, const float *src_b, int64_t n_b,
                                   const float *z, int32_t obs_dim, int32_t latent_dim, float *rows_out, void *stream) {
    if (int rc = bcq_check("tsm_bcq_decode_rows", 1, latent_dim, rep_a)) return rc;
    TSM_REQUIRE(obs_dim >= 1 && n_a >= 1 && n_b >= 0 && rep_a <= (1 << 20) && n_a < ((int64_t)1 << 31) && n_b < ((int64_t)1 << 31),
                "tsm_bcq_decode_rows: obs_dim = %d, n_a = %lld (at least 1 each), n_b = %lld (at least 0), rep_a = %d", obs_dim,
                (long long)n_a, (long long)n_b, rep_a);
    if (int rc = bcq_check_rows("tsm_bcq_decode_rows", n_a * rep_a + n_b, (int64_t)obs_dim + latent_dim)) return rc;
    TSM_REQUIRE(src_a && z && rows_out && (n_b == 0 || src_b), "tsm_bcq_decode_rows: null pointer");
    hipLaunchKernelGGL(bcq_decode_rows_kernel, bcq_grid((n_a * rep_a + n_b) * ((int64_t)obs_dim + latent_dim)), dim3(kBThreads), 0,
                       tsm_stream(stream), src_a, n_a, (int64_t)rep_a, src_b, n_b, z, obs_dim, latent_dim, rows_out);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_bcq_action_rows(const float *raw, const float *x_dec, int64_t n, int32_t obs_dim, int32_t latent_dim,
                                   int32_t act_dim, double max_action, float *x_out, void *stream) {
    if (int rc = bcq_check("tsm_bcq_action_rows", act_dim, latent_dim, 1)) return rc;
    TSM_REQUIRE(obs_dim >= 1, "tsm_bcq_action_rows: obs_dim = %d below 1", obs_dim);
    if (int rc = bcq_check_rows("tsm_bcq_action_rows", n, (int64_t)obs_dim + latent_dim + act_dim)) return rc;
    TSM_REQUIRE(raw && x_dec && x_out, "tsm_bcq_action_rows: null pointer");
    hipLaunchKernelGGL(bcq_action_rows_kernel, bcq_grid(n * ((int64_t)obs_dim + act_dim)), dim3(kBThreads), 0, tsm_stream(stream),
                       raw, x_dec, n, obs_dim, latent_dim, act_dim, max_action, x_out);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_bcq_target(const float *q1, const float *q2, const float *rew, const uint8_t *vmask, int64_t B,
                              int32_t num_sampled, double gamma, double lmbda, float *target_out, void *stream) {
    TSM_REQUIRE(num_sampled >= 1, "tsm_bcq_target: the number of sampled actions should be at least 1 but got: %d", num_sampled);
    if (int rc = bcq_check_rows("tsm_bcq_target", B, num_sampled)) return rc;
    TSM_REQUIRE(q1 && q2 && rew && vmask && target_out, "tsm_bcq_target: null pointer");
    // logical_not(done) * gamma is a float32 tensor in the reference (bcq.py:235): gamma enters the product rounded to float32
    hipLaunchKernelGGL(bcq_target_kernel, dim3((unsigned)ceil_div(B, kBThreads)), dim3(kBThreads), 0, tsm_stream(stream), q1, q2,
                       rew, vmask, B, (int64_t)num_sampled, (double)(float)gamma, lmbda, target_out);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_bcq_vae_head(const float *raw_dec, const float *act, const float *head, int64_t B, int32_t act_dim,
                                int32_t latent_dim, double max_action, float *d_raw_out, double *partial, void *stream) {
    if (int rc = bcq_check("tsm_bcq_vae_head", act_dim, latent_dim, 1)) return rc;
    if (int rc = tsm_q_check_rows("tsm_bcq_vae_head", B)) return rc;
    TSM_REQUIRE(raw_dec && act && head && d_raw_out && partial, "tsm_bcq_vae_head: null pointer");
    hipLaunchKernelGGL(bcq_vae_head_kernel, dim3((unsigned)ceil_div(B, TSM_CAC_ROWS_PER_BLOCK)), dim3(kBThreads), 0,
                       tsm_stream(stream), raw_dec, act, head, B, act_dim, latent_dim, max_action, d_raw_out, partial);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_bcq_latent_grad(const float *dz, const float *head, const float *eps, int64_t B, int32_t latent_dim,
                                   float *d_head_out, void *stream) {
    if (int rc = bcq_check("tsm_bcq_latent_grad", 1, latent_dim, 1)) return rc;
    if (int rc = bcq_check_rows("tsm_bcq_latent_grad", B, 2 * (int64_t)latent_dim)) return rc;
    TSM_REQUIRE(dz && head && eps && d_head_out, "tsm_bcq_latent_grad: null pointer");
    hipLaunchKernelGGL(bcq_latent_grad_kernel, bcq_grid(B * latent_dim), dim3(kBThreads), 0, tsm_stream(stream), dz, head, eps, B,
                       latent_dim, d_head_out);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_bcq_perturb(const float *raw_p, const float *x_in, int64_t n, int32_t obs_dim, int32_t act_dim, double phi,
                               double max_action, float *x_out, float *factor_out, void *stream) {
    if (int rc = bcq_check("tsm_bcq_perturb", act_dim, 1, 1)) return rc;
    TSM_REQUIRE(obs_dim >= 1, "tsm_bcq_perturb: obs_dim = %d below 1", obs_dim);
    if (int rc = bcq_check_rows("tsm_bcq_perturb", n, (int64_t)obs_dim + act_dim)) return rc;
    TSM_REQUIRE(raw_p && x_in && x_out, "tsm_bcq_perturb: null pointer");
    TSM_REQUIRE(x_in != x_out, "tsm_bcq_perturb: x_out must not be x_in");
    hipLaunchKernelGGL(bcq_perturb_kernel, bcq_grid(n * ((int64_t)obs_dim + act_dim)), dim3(kBThreads), 0, tsm_stream(stream),
                       raw_p, x_in, n, obs_dim, act_dim, phi, max_action, x_out, factor_out);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_bcq_select(const float *q, const float *rows, int64_t ld, int32_t col0, int64_t n, int32_t num_sampled,
                              int32_t act_dim, float *act_out, int32_t *index_out, void *stream) {
    if (int rc = bcq_check("tsm_bcq_select", act_dim, 1, num_sampled)) return rc;
    TSM_REQUIRE(col0 >= 0 && (int64_t)col0 + act_dim <= ld, "tsm_bcq_select: columns [%d, %d) leave the row of %lld floats", col0,
                col0 + act_dim, (long long)ld);
    TSM_REQUIRE(n >= 1 && n < ((int64_t)1 << 31) && num_sampled <= (1 << 20), "tsm_bcq_select: n = %lld groups of %d", (long long)n,
                num_sampled);
    if (int rc = bcq_check_rows("tsm_bcq_select", n * num_sampled, ld)) return rc;
    TSM_REQUIRE(q && rows && act_out && index_out, "tsm_bcq_select: null pointer");
    hipLaunchKernelGGL(bcq_select_kernel, dim3((unsigned)ceil_div(n, kBWaves)), dim3(kBThreads), 0, tsm_stream(stream), q, rows,
                       ld, col0, n, num_sampled, act_dim, act_out, index_out);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}
