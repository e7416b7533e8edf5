// maddpg.hip -- MADDPG: joint-row assembly for the centralized critics, the per-agent TD head, the loss finalize, the
// acting epilogue (exploration noise + clamp) and the soft target update.
//
// Replaces, in MADDPGPolicy (/root/reference/tianshou/algorithm/multiagent/ctde.py:728-955):
//   the torch.cat chains that build the critics' inputs                         :875-880, :888, :893, :913-919
//   td_target / F.mse_loss and its gradient w.r.t. q                             :895-898 (+ the head of :902)
//   actor_loss = -critic(...).mean(), the .item() reads and the np.mean's        :918-920, :927-932
//   update_target_networks                                                       :936-955
// The actors and critics run in csrc/dense.hip (tsm_mlp_forward / tsm_mlp_backward / tsm_mlp_input_grad).
//
// Within one learn call the agents are independent (critic i and actor i read the batch, the TARGET actors, target critic
// i, critic i and actor i only -- the actors stepped earlier in the reference's loop are never read again), so every kernel
// here serves all N agents in one launch.
#include "common.h"
#include "philox.h"

namespace {
constexpr int kMThreads = 256;
constexpr int kMMaxN = TSM_MADDPG_MAX_AGENTS;
constexpr int kJoinRows = 16;  // joint rows per workgroup of the assembly kernel

struct JoinPtrs { const float *obs[kMMaxN]; const float *act[kMMaxN]; const float *rep[kMMaxN]; };
struct ActPtrs { const float *mu[kMMaxN]; };
struct FinPtrs { const float *q_pi[kMMaxN]; };

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// One region of the joint rows: n_seg segments of `w` floats per row, segment j of row b read from src_j[b * w ..] and
// written to out[b * W + c0 + j * w ..].  Lanes run along the row (consecutive lanes, consecutive addresses on both sides).
// VEC: w, c0 and W are multiples of 4 and every pointer is 16-B aligned (decided on the host) -> 16-B accesses.
template <bool VEC>
__device__ __forceinline__ void join_region(const float *const *src, const float *rep, int rep_seg, int n_seg, int w, int c0,
                                            int64_t W, int64_t b0, int nr, float *__restrict__ out) {
    const int rw = n_seg * w;  // floats of this region per row
    if (VEC) {
        const int rw4 = rw >> 2, n4 = nr * rw4;
        for (int q = threadIdx.x; q < n4; q += kMThreads) {
            const int r = q / rw4, c = (q - r * rw4) * 4, j = c / w, k = c - j * w;
            const float *s = (j == rep_seg) ? rep : src[j];
            st4(out + (b0 + r) * W + c0 + c, ld4(s + (b0 + r) * w + k));
        }
    } else {
        const int n = nr * rw;
        for (int q = threadIdx.x; q < n; q += kMThreads) {
            const int r = q / rw, c = q - r * rw, j = c / w, k = c - j * w;
            const float *s = (j == rep_seg) ? rep : src[j];
            out[(b0 + r) * W + c0 + c] = s[(b0 + r) * w + k];
        }
    }
}

// grid (ceil(B / kJoinRows), M): matrix m = blockIdx.y of out[M][B][W]; with `rep` pointers matrix m carries rep[m] in
// agent m's action slot, without them M = 1 and the rows are the batch's own
__global__ __launch_bounds__(kMThreads) void maddpg_joint_rows_kernel(JoinPtrs p, int N, int D, int Ad, int64_t B, int has_rep,
                                                                      int vec_obs, int vec_act, float *__restrict__ out) {
    const int m = blockIdx.y;
    const int64_t W = (int64_t)N * (D + Ad);
    const int64_t b0 = (int64_t)blockIdx.x * kJoinRows;
    const int nr = (int)(B - b0 < kJoinRows ? B - b0 : kJoinRows);
    float *dst = out + (int64_t)m * B * W;
    if (vec_obs) join_region<true>(p.obs, nullptr, -1, N, D, 0, W, b0, nr, dst);
    else join_region<false>(p.obs, nullptr, -1, N, D, 0, W, b0, nr, dst);
    const float *rep = has_rep ? p.rep[m] : nullptr;
    const int rs = has_rep ? m : -1;
    if (vec_act) join_region<true>(p.act, rep, rs, N, Ad, N * D, W, b0, nr, dst);
    else join_region<false>(p.act, rep, rs, N, Ad, N * D, W, b0, nr, dst);
}

// one thread per joint row, all agents: y_i = rew_i + gamma q'_i (1 - term_i), d = q_i - y_i, dq_i = 2 d / B, formed in f64
// from the f32 inputs and rounded once (q_i - y_i cancels: in f32 the rounding of y_i alone is many ulp of a small d);
// partial[blockIdx.x * N + i] = sum over the block's rows of d^2 in f64 (wave butterfly, then the waves in order)
__global__ __launch_bounds__(kMThreads) void maddpg_td_kernel(tsm_maddpg_agents ag, int N, int64_t B, double gamma,
                                                              double *__restrict__ partial) {
    __shared__ double s_red[kMThreads / kWave];
    const int64_t b = (int64_t)blockIdx.x * kMThreads + threadIdx.x;
    const bool valid = b < B;
    for (int i = 0; i < N; ++i) {
        double sq = 0.0;
        if (valid) {
            const double nt = ag.term[i][b] ? 0.0 : 1.0;
            const double y = (double)ag.rew[i][b] + gamma * (double)ag.q_next[i][b] * nt;
            const double d = (double)ag.q[i][b] - y;
            ag.dq[i][b] = (float)(2.0 * d / (double)B);
            sq = d * d;
        }
        const double tot = block_sum<double, kMThreads>(sq, s_red);
        if (threadIdx.x == 0) partial[(int64_t)blockIdx.x * N + i] = tot;
    }
}

// block i: critic MSE of agent i from the TD partials and -mean(q_pi[i]); thread t takes entries t, t + 256, ... then the
// block sum -- a fixed order.  out[2 i] = actor_loss_i, out[2 i + 1] = critic_loss_i.
__global__ __launch_bounds__(kMThreads) void maddpg_finalize_kernel(const double *__restrict__ partial, int nb, int N,
                                                                    FinPtrs fp, int64_t B, float *__restrict__ out) {
    __shared__ double s_red[kMThreads / kWave];
    const int i = blockIdx.x;
    double sq = 0.0, sp = 0.0;
    for (int k = threadIdx.x; k < nb; k += kMThreads) sq += partial[(int64_t)k * N + i];
    const float *q = fp.q_pi[i];
    for (int64_t b = threadIdx.x; b < B; b += kMThreads) sp += (double)q[b];
    sq = block_sum<double, kMThreads>(sq, s_red);
    sp = block_sum<double, kMThreads>(sp, s_red);
    if (threadIdx.x != 0) return;
    out[2 * i] = (float)(-sp / (double)B);
    out[2 * i + 1] = (float)(sq / (double)B);
}

// element idx of out[E * N][Ad] (row e * N + i = env e, agent i) <- mu_i[e][k] (+ sigma z) (clamped to [low[k], high[k]]);
// z: Box-Muller on words 0 and 1 of Philox(seed, c + idx).  sigma == 0 and no bounds: the actor's bits.
__global__ __launch_bounds__(kMThreads) void maddpg_act_kernel(ActPtrs ap, int N, int Ad, int64_t E,
                                                               const float *__restrict__ sigma_dev, uint64_t seed,
                                                               uint64_t offset, const uint64_t *__restrict__ offset_dev,
                                                               const float *__restrict__ low, const float *__restrict__ high,
                                                               float *__restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * kMThreads + threadIdx.x;
    if (idx >= E * N * Ad) return;
    const int64_t row = idx / Ad;
    const int k = (int)(idx - row * Ad);
    const int64_t e = row / N;
    const int i = (int)(row - e * N);
    float v = ap.mu[i][e * Ad + k];
    const float sigma = *sigma_dev;
    if (sigma != 0.f) {
        const uint64_t c = offset + (offset_dev ? *offset_dev : 0ull);
        uint32_t bits[4];
        tsm_philox4(seed, c + (uint64_t)idx, bits);
        const float u1 = 1.f - tsm_u01(bits[0]);  // (0, 1]
        const float u2 = tsm_u01(bits[1]);
        const float z = sqrtf(-2.f * logf(u1)) * cosf(6.28318530717958647692f * u2);
        v = v + sigma * z;
    }
    if (low) v = fminf(fmaxf(v, low[k]), high[k]);
    out[idx] = v;
}

// target = tau p + (1 - tau) target: two rounded f32 products, then their rounded sum (what the torch expression gives)
__device__ __forceinline__ float polyak1(float a, float b, float p, float t) {
    return __fadd_rn(__fmul_rn(a, p), __fmul_rn(b, t));
}
__global__ __launch_bounds__(kMThreads) void polyak_kernel(float *__restrict__ target, const float *__restrict__ p, int64_t n,
                                                           float a, float b, int vec) {
    const int64_t t = (int64_t)blockIdx.x * kMThreads + threadIdx.x;
    if (vec) {
        const int64_t n4 = n >> 2;
        if (t < n4) {
            const float4 x = ld4(p + 4 * t), y = ld4(target + 4 * t);
            st4(target + 4 * t, make_float4(polyak1(a, b, x.x, y.x), polyak1(a, b, x.y, y.y), polyak1(a, b, x.z, y.z),
                                            polyak1(a, b, x.w, y.w)));
        }
        const int64_t j = 4 * n4 + t;  // the up to 3 elements behind the last whole quad
        if (t < 3 && j < n) target[j] = polyak1(a, b, p[j], target[j]);
    } else if (t < n) {
        target[t] = polyak1(a, b, p[t], target[t]);
    }
}

int check_sizes(const char *who, int32_t N, int64_t B) {
    TSM_REQUIRE(N >= 1 && N <= kMMaxN, "%s: n_agents = %d outside [1, %d]", who, N, kMMaxN);
    TSM_REQUIRE(B >= 1 && B <= ((int64_t)1 << 31) - 1, "%s: B = %lld out of range", who, (long long)B);
    return TSM_OK;
}
}  // namespace

TSM_EXPORT int tsm_maddpg_joint_rows(const float *const *obs_by_agent_host, const float *const *act_by_agent_host,
                                     const float *const *replace_by_agent_host, int32_t n_agents, int64_t B, int32_t D,
                                     int32_t Ad, float *out, void *stream) {
    if (int rc = check_sizes("tsm_maddpg_joint_rows", n_agents, B)) return rc;
    TSM_REQUIRE(D >= 1 && D <= (1 << 16), "tsm_maddpg_joint_rows: obs_dim = %d outside [1, 65536]", D);
    TSM_REQUIRE(Ad >= 1 && Ad <= (1 << 16), "tsm_maddpg_joint_rows: act_dim = %d outside [1, 65536]", Ad);
    TSM_REQUIRE(obs_by_agent_host && act_by_agent_host && out, "tsm_maddpg_joint_rows: null pointer");
    const int64_t W = (int64_t)n_agents * (D + Ad);
    // a workgroup indexes its kJoinRows x W piece with ints
    TSM_REQUIRE(W * kJoinRows < ((int64_t)1 << 31), "tsm_maddpg_joint_rows: joint row of %lld floats is too wide", (long long)W);
    JoinPtrs p{};
    bool al_obs = aligned16(out), al_act = aligned16(out);
    for (int i = 0; i < n_agents; ++i) {
        TSM_REQUIRE(obs_by_agent_host[i] && act_by_agent_host[i], "tsm_maddpg_joint_rows: null pointer for agent %d", i);
        TSM_REQUIRE(!replace_by_agent_host || replace_by_agent_host[i], "tsm_maddpg_joint_rows: null replacement for agent %d", i);
        p.obs[i] = obs_by_agent_host[i];
        p.act[i] = act_by_agent_host[i];
        p.rep[i] = replace_by_agent_host ? replace_by_agent_host[i] : nullptr;
        al_obs = al_obs && aligned16(p.obs[i]);
        al_act = al_act && aligned16(p.act[i]) && (!p.rep[i] || aligned16(p.rep[i]));
    }
    const int M = replace_by_agent_host ? n_agents : 1;
    // matrix m starts at m * B * W floats: 16-B aligned for every m only when B * W is a multiple of 4 (W % 4 == 0 gives it)
    const int vec_obs = al_obs && W % 4 == 0 && D % 4 == 0;
    const int vec_act = al_act && W % 4 == 0 && Ad % 4 == 0 && ((int64_t)n_agents * D) % 4 == 0;
    dim3 grid((unsigned)ceil_div(B, kJoinRows), (unsigned)M, 1);
    hipLaunchKernelGGL(maddpg_joint_rows_kernel, grid, dim3(kMThreads), 0, tsm_stream(stream), p, n_agents, D, Ad, B,
                       replace_by_agent_host ? 1 : 0, vec_obs, vec_act, out);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int64_t tsm_maddpg_partial_elems(int64_t B, int32_t n_agents) {
    if (B < 1 || n_agents < 1 || n_agents > kMMaxN) return -1;
    return (int64_t)n_agents * ceil_div(B, kMThreads);
}

TSM_EXPORT int tsm_maddpg_td(const tsm_maddpg_agents *agents, int32_t n_agents, int64_t B, double gamma, double *partial,
                             void *stream) {
    if (int rc = check_sizes("tsm_maddpg_td", n_agents, B)) return rc;
    TSM_REQUIRE(agents && partial, "tsm_maddpg_td: null pointer");
    for (int i = 0; i < n_agents; ++i)
        TSM_REQUIRE(agents->q[i] && agents->q_next[i] && agents->rew[i] && agents->term[i] && agents->dq[i],
                    "tsm_maddpg_td: null pointer for agent %d", i);
    hipLaunchKernelGGL(maddpg_td_kernel, dim3((unsigned)ceil_div(B, kMThreads)), dim3(kMThreads), 0, tsm_stream(stream),
                       *agents, n_agents, B, gamma, partial);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_maddpg_finalize(const double *partial, int32_t n_blocks, const float *const *q_pi_by_agent_host,
                                   int32_t n_agents, int64_t B, float *out, void *stream) {
    if (int rc = check_sizes("tsm_maddpg_finalize", n_agents, B)) return rc;
    TSM_REQUIRE(n_blocks >= 1, "tsm_maddpg_finalize: n_blocks = %d must be >= 1", n_blocks);
    TSM_REQUIRE(partial && q_pi_by_agent_host && out, "tsm_maddpg_finalize: null pointer");
    FinPtrs fp{};
    for (int i = 0; i < n_agents; ++i) {
        TSM_REQUIRE(q_pi_by_agent_host[i], "tsm_maddpg_finalize: null pointer for agent %d", i);
        fp.q_pi[i] = q_pi_by_agent_host[i];
    }
    hipLaunchKernelGGL(maddpg_finalize_kernel, dim3((unsigned)n_agents), dim3(kMThreads), 0, tsm_stream(stream), partial,
                       n_blocks, n_agents, fp, B, out);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_maddpg_act(const float *const *mu_by_agent_host, int32_t n_agents, int64_t E, int32_t Ad,
                              const float *sigma_dev, uint64_t seed, uint64_t offset, const uint64_t *offset_dev,
                              const float *low, const float *high, float *act_out, void *stream) {
    TSM_REQUIRE(n_agents >= 1 && n_agents <= kMMaxN, "tsm_maddpg_act: n_agents = %d outside [1, %d]", n_agents, kMMaxN);
    TSM_REQUIRE(Ad >= 1 && Ad <= (1 << 16), "tsm_maddpg_act: act_dim = %d outside [1, 65536]", Ad);
    TSM_REQUIRE(E >= 0 && E * n_agents * Ad < ((int64_t)1 << 31) * kMThreads, "tsm_maddpg_act: E = %lld out of range", (long long)E);
    TSM_REQUIRE((low == nullptr) == (high == nullptr), "tsm_maddpg_act: low and high bounds come together");
    if (E == 0) return TSM_OK;
    TSM_REQUIRE(mu_by_agent_host && sigma_dev && act_out, "tsm_maddpg_act: null pointer");
    ActPtrs ap{};
    for (int i = 0; i < n_agents; ++i) {
        TSM_REQUIRE(mu_by_agent_host[i], "tsm_maddpg_act: null actor output for agent %d", i);
        ap.mu[i] = mu_by_agent_host[i];
    }
    hipLaunchKernelGGL(maddpg_act_kernel, dim3((unsigned)ceil_div(E * n_agents * Ad, kMThreads)), dim3(kMThreads), 0,
                       tsm_stream(stream), ap, n_agents, Ad, E, sigma_dev, seed, offset, offset_dev, low, high, act_out);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_polyak(float *target, const float *param, int64_t n, double tau, void *stream) {
    TSM_REQUIRE(n >= 0 && n < ((int64_t)1 << 31) * kMThreads, "tsm_polyak: n = %lld out of range", (long long)n);
    TSM_REQUIRE(tau >= 0.0 && tau <= 1.0, "tsm_polyak: tau = %g outside [0, 1]", tau);
    if (n == 0) return TSM_OK;
    TSM_REQUIRE(target && param, "tsm_polyak: null pointer");
    const int vec = aligned16(target) && aligned16(param);
    const int64_t threads = vec ? (n / 4 > 3 ? n / 4 : 3) : n;
    hipLaunchKernelGGL(polyak_kernel, dim3((unsigned)ceil_div(threads, kMThreads)), dim3(kMThreads), 0, tsm_stream(stream),
                       target, param, n, (float)tau, (float)(1.0 - tau), vec);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}
