// bdqn.hip -- BDQN (arXiv 1711.08946): the per-branch dueling combine, the branch-mean target with the masked TD loss and its
// backward, and per-branch epsilon-greedy acting.
//
// Replaces, in tianshou/utils/net/common.py and tianshou/algorithm/modelfree/bdqn.py:
//   BranchingNet.forward after its MLPs (stack, subtract the branch's mean, add the value)            common.py:669-677
//   BDQN._target_q after its forwards, _compute_return, and _update_with_batch between
//     `self.policy(batch).logits` and `optim.step`                                                    bdqn.py:155-171, 173-195, 211-221
//   BDQNPolicy.forward's argmax and add_exploration_noise                                            bdqn.py:76, 80-103
// The trunk and the value stream run in csrc/dense.hip, the K branches in csrc/ensemble.hip (one grouped launch per layer).
//
// Layouts: adv f32 [K][B][A] (the ensemble's output block), v f32 [B], q f32 [B][K][A] (the reference's logits), act i32 [B][K].
// Arithmetic is f64 from the f32 inputs; every sum has a fixed order (a' = 0 .. A - 1, k = 0 .. K - 1, then the workgroup's
// rows in order); no atomics, so two runs give the same bits.
//
// Head: a workgroup of 256 threads owns TSM_BDQN_ROWS_PER_BLOCK = 16 rows.  Its threads stride over the (row, branch) pairs
// -- at most 16 * 64 -- three times, with LDS between the passes:
//   pass 1  pair (r, k): a*_k = first maximum of q_next_online[b][k][:] (is_double) or of the target values, s_tv = target[b][k][a*_k]
//   fold 1  thread r < 16: tq = mean_k s_tv in k order;  returns[b] = rew + gamma tq (1 - end), rounded once
//   pass 2  pair (r, k): td = returns[b] - q[b][k][act[b][k]];  g = -2 w td / (K B);  d_adv[k][b][a] = g ((a == act) - 1 / A)
//   fold 2  thread r < 16: prio = sum_k td, l = w mean_k td^2, d_v = sum_k g, in k order; threads 0 and 1 add the 16 rows in
//           order into the workgroup's pair {sum l, sum mean_k q_taken} (tsm_qmix_mix_td's layout, for tsm_qmix_finalize)
// An act entry outside [0, A) reads nothing: its td is NaN (the loss and the row's priority are poisoned), its d_adv row and
// its share of d_v are 0 -- as tsm_dqn_td_head zeroes the gradient row of such an action.
#include "common.h"
#include "philox.h"
#include "q_head_dev.h"

namespace {
constexpr int kBThreads = 256;
constexpr int kBRows = TSM_BDQN_ROWS_PER_BLOCK;
constexpr int kBMaxK = TSM_ENS_MAX_MEMBERS;

// one thread per element of q; the A values of its (b, k) row are summed by each of the row's threads, in order
__global__ __launch_bounds__(kBThreads) void bdqn_combine_kernel(const float *__restrict__ adv, const float *__restrict__ v,
                                                                 int64_t B, int32_t K, int32_t A, float *__restrict__ q) {
    const int64_t i = (int64_t)blockIdx.x * kBThreads + threadIdx.x;
    if (i >= B * K * A) return;
    const int a = (int)(i % A);
    const int64_t bk = i / A;
    const int k = (int)(bk % K);
    const int64_t b = bk / K;
    const float *row = adv + ((int64_t)k * B + b) * A;
    double s = 0.0;
    for (int j = 0; j < A; ++j) s += (double)row[j];
    q[i] = (float)((double)v[b] + ((double)row[a] - s / (double)A));
}

__global__ __launch_bounds__(kBThreads) void bdqn_head_kernel(
    const float *__restrict__ q, const float *__restrict__ qn_on, const float *__restrict__ qn_tg, const int32_t *__restrict__ act,
    const float *__restrict__ rew, const uint8_t *__restrict__ end, const float *__restrict__ weight, int64_t B, int32_t K,
    int32_t A, double gamma, int is_double, float *__restrict__ returns_out, float *__restrict__ prio, float *__restrict__ d_adv,
    float *__restrict__ d_v, double *__restrict__ partial) {
    __shared__ float s_tv[kBRows][kBMaxK];
    __shared__ double s_td[kBRows][kBMaxK];   // NaN for an action outside [0, A)
    __shared__ float s_qs[kBRows][kBMaxK];
    __shared__ float s_ret[kBRows];
    __shared__ double s_row[2][kBRows];
    const int t = threadIdx.x;
    const int64_t b0 = (int64_t)blockIdx.x * kBRows;
    const int rows = (int)(B - b0 < kBRows ? B - b0 : kBRows);
    const int pairs = rows * K;
    const float *qt = qn_tg ? qn_tg : qn_on;
    const float *qsel = is_double ? qn_on : qt;

    for (int p = t; p < pairs; p += kBThreads) {
        const int r = p / K, k = p - r * K;
        const int64_t o = ((b0 + r) * K + k) * A;
        s_tv[r][k] = qt[o + tsm_q_first_argmax(qsel + o, nullptr, A, 0.f)];
    }
    __syncthreads();
    if (t < rows) {
        const int64_t b = b0 + t;
        double s = 0.0;
        for (int k = 0; k < K; ++k) s += (double)s_tv[t][k];
        const double tq = s / (double)K;
        const float ret = (float)((double)rew[b] + gamma * tq * (end[b] ? 0.0 : 1.0));
        s_ret[t] = ret;
        returns_out[b] = ret;
    }
    __syncthreads();
    const double n = (double)K * (double)B;
    for (int p = t; p < pairs; p += kBThreads) {
        const int r = p / K, k = p - r * K;
        const int64_t b = b0 + r;
        const int32_t ac = act[b * K + k];
        const bool ok = ac >= 0 && ac < A;
        const float qs = ok ? q[(b * K + k) * A + ac] : __builtin_nanf("");
        const double td = (double)s_ret[r] - (double)qs;
        const double wt = weight ? (double)weight[b] : 1.0;
        const double g = -2.0 * wt * td / n;
        s_td[r][k] = td;
        s_qs[r][k] = qs;
        float *drow = d_adv + ((int64_t)k * B + b) * A;
        const double inv_a = 1.0 / (double)A;
        for (int a = 0; a < A; ++a) drow[a] = ok ? (float)(g * ((a == ac ? 1.0 : 0.0) - inv_a)) : 0.f;
    }
    __syncthreads();
    if (t < rows) {
        const int64_t b = b0 + t;
        const double wt = weight ? (double)weight[b] : 1.0;
        double s_t = 0.0, s_t2 = 0.0, s_g = 0.0, s_q = 0.0;
        for (int k = 0; k < K; ++k) {
            const double td = s_td[t][k];
            s_t += td;
            s_t2 += td * td;
            const int32_t ac = act[b * K + k];
            if (ac >= 0 && ac < A) s_g += -2.0 * wt * td / n;
            s_q += (double)s_qs[t][k];
        }
        prio[b] = (float)s_t;
        d_v[b] = (float)s_g;
        s_row[0][t] = wt * (s_t2 / (double)K);
        s_row[1][t] = s_q / (double)K;
    }
    __syncthreads();
    if (t < 2) {
        double acc = 0.0;
        for (int r = 0; r < rows; ++r) acc += s_row[t][r];
        partial[(int64_t)blockIdx.x * 2 + t] = acc;
    }
}

// One thread per (row, branch).  Draws of row r are words of Philox4x32-10 at (seed, counter c + r): the coin is word 0 of
// sub 0, read by each of the row's K threads; branch k's action is word k % 4 of sub 1 + k / 4, times A, high half.
__global__ __launch_bounds__(kBThreads) void bdqn_egreedy_kernel(const float *__restrict__ q, int64_t R, int32_t K, int32_t A,
                                                                 const float *__restrict__ eps_dev, uint64_t seed, uint64_t offset,
                                                                 const uint64_t *__restrict__ offset_dev,
                                                                 int32_t *__restrict__ act) {
    const int64_t i = (int64_t)blockIdx.x * kBThreads + threadIdx.x;
    if (i >= R * K) return;
    const int64_t r = i / K;
    const int k = (int)(i - r * K);
    const uint64_t c = offset + (offset_dev ? *offset_dev : 0ull) + (uint64_t)r;
    uint32_t bits[4];
    tsm_philox4(seed, c, bits);
    int a_sel;
    if (tsm_u01(bits[0]) < *eps_dev) {   // rand(bsz) < eps, then randint(0, A) per branch   (bdqn.py:90-95)
        tsm_philox4_sub(seed, c, 1u + (uint32_t)(k >> 2), bits);
        a_sel = (int)(((uint64_t)bits[k & 3] * (uint64_t)A) >> 32);
    } else {
        a_sel = tsm_q_first_argmax(q + i * A, nullptr, A, 0.f);
    }
    act[i] = a_sel;
}

int bdqn_check(const char *who, int32_t K, int32_t A) {
    TSM_REQUIRE(K >= 1 && K <= TSM_ENS_MAX_MEMBERS, "%s: num_branches = %d outside [1, %d]", who, K, TSM_ENS_MAX_MEMBERS);
    return tsm_q_check_act(who, A);
}
}  // namespace

TSM_EXPORT int tsm_bdqn_check(int32_t K, int32_t A) { return bdqn_check("tsm_bdqn_check", K, A); }

TSM_EXPORT int tsm_bdqn_combine(const float *adv, const float *v, int64_t B, int32_t K, int32_t A, float *q, void *stream) {
    if (int rc = bdqn_check("tsm_bdqn_combine", K, A)) return rc;
    if (int rc = tsm_q_check_rows("tsm_bdqn_combine", B)) return rc;   // B K A stays below 2^43: 64-bit offsets, a grid below 2^31
    TSM_REQUIRE(adv && v && q, "tsm_bdqn_combine: null pointer");
    hipLaunchKernelGGL(bdqn_combine_kernel, dim3((unsigned)ceil_div(B * K * A, kBThreads)), dim3(kBThreads), 0, tsm_stream(stream),
                       adv, v, B, K, A, q);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_bdqn_head(const float *q, const float *q_next_online, const float *q_next_target, const int32_t *act,
                             const float *rew, const uint8_t *end, const float *weight, int64_t B, int32_t K, int32_t A,
                             double gamma, int is_double, float *returns_out, float *prio, float *d_adv, float *d_v,
                             double *partial, void *stream) {
    if (int rc = bdqn_check("tsm_bdqn_head", K, A)) return rc;
    if (int rc = tsm_q_check_rows("tsm_bdqn_head", B)) return rc;
    TSM_REQUIRE(q && q_next_online && act && rew && end && returns_out && prio && d_adv && d_v && partial,
                "tsm_bdqn_head: null pointer");
    hipLaunchKernelGGL(bdqn_head_kernel, dim3((unsigned)ceil_div(B, kBRows)), dim3(kBThreads), 0, tsm_stream(stream), q,
                       q_next_online, q_next_target, act, rew, end, weight, B, K, A, gamma, is_double, returns_out, prio, d_adv,
                       d_v, partial);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_bdqn_egreedy(const float *q, int64_t R, int32_t K, int32_t A, const float *eps_dev, uint64_t seed,
                                uint64_t offset, const uint64_t *offset_dev, int32_t *act_out, void *stream) {
    if (int rc = bdqn_check("tsm_bdqn_egreedy", K, A)) return rc;
    TSM_REQUIRE(R >= 0 && R <= ((int64_t)1 << 31) / kQHeadMaxA, "tsm_bdqn_egreedy: R = %lld out of range", (long long)R);
    if (R == 0) return TSM_OK;
    TSM_REQUIRE(q && eps_dev && act_out, "tsm_bdqn_egreedy: null pointer");
    hipLaunchKernelGGL(bdqn_egreedy_kernel, dim3((unsigned)ceil_div(R * K, kBThreads)), dim3(kBThreads), 0, tsm_stream(stream), q,
                       R, K, A, eps_dev, seed, offset, offset_dev, act_out);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}
