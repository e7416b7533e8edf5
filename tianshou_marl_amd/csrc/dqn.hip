// dqn.hip -- DQN: the bootstrap value, the n-step target, the TD loss with its backward, and masked epsilon-greedy acting.
//
// Replaces DQN._target_q and the arithmetic of DQN._update_with_batch between the network forwards and `optim.step(loss)`
// (/root/reference/tianshou/algorithm/modelfree/dqn.py:365-404), the last line of `_nstep_return`
// (algorithm_base.py:1213-1215) and, on the device, DiscreteQLearningPolicy.forward's action choice with
// add_exploration_noise (dqn.py:140-141, 153-171).  The Q-networks run in csrc/dense.hip, the n-step walk in csrc/nstep.hip.
//
// Per row b (one thread):
//   qt      = q_next_target, or q_next_online when there is no target network
//   double: a* = first argmax_a (q_next_online[b][a] + (1 - mask[b][a]) * mv),  target = qt[b][a*]
//           mv = min(q_next_online) - max(q_next_online) - 1 over the WHOLE [B][A] tensor (compute_q_value, dqn.py:147-150):
//           every workgroup reduces the tensor itself (min and max do not depend on the order, so all agree bit for bit);
//           without a mask no offset is applied and the reduction is skipped
//   else:   target = max_a qt[b][a]                      (the mask does not enter: dqn.py:379 takes the raw maximum)
//   returns = target * vmask * gpow + mc  in float64, rounded once (numpy's f32 * f64 + f64, then to_torch_as)
//   td      = returns - q[b][act[b]]
//   MSE:    l = td^2 w[b]                                d q[b][act] = -2 td w[b] / B
//   Huber:  e = -td; l = |e| < delta ? e^2 / 2 : delta (|e| - delta / 2);   d q[b][act] = clamp(e, -delta, delta) / B
//           (`weight` does not enter the Huber loss: dqn.py:392-397 drops it)
// Loss and mean(q[b][act]) leave as per-workgroup f64 partials in tsm_qmix_mix_td's layout {sum l, sum q}, so
// tsm_qmix_finalize turns them into {loss, mean q} in a pinned slot.
#include "common.h"
#include "philox.h"
#include "q_head_dev.h"

namespace {
constexpr int kDThreads = TSM_DQN_ROWS_PER_BLOCK;

__global__ __launch_bounds__(kDThreads) void dqn_td_head_kernel(
    const float *__restrict__ q, const float *__restrict__ qn_on, const float *__restrict__ qn_tg,
    const uint8_t *__restrict__ mask_next, const int64_t *__restrict__ act, const float *__restrict__ mc,
    const float *__restrict__ gpow, const uint8_t *__restrict__ vmask, const float *__restrict__ weight, int64_t B,
    int32_t A, int is_double, float huber_delta, float *__restrict__ returns_out, float *__restrict__ td_out,
    float *__restrict__ dq, double *__restrict__ partial) {
    __shared__ float s_min[kDThreads / kWave], s_max[kDThreads / kWave];
    __shared__ double s_red[2][kDThreads / kWave];
    const int t = threadIdx.x, lane = t & (kWave - 1), w = t / kWave;
    const bool masked = is_double && mask_next != nullptr;

    // logits.min() - logits.max() - 1 over the whole tensor (q_head_dev.h)
    const float mv = masked ? tsm_q_mask_offset<kDThreads>(qn_on, B * A, s_min, s_max) : 0.f;

    const int64_t b = (int64_t)blockIdx.x * kDThreads + t;
    double p_l = 0.0, p_q = 0.0;
    if (b < B) {
        const float *qt = (qn_tg ? qn_tg : qn_on) + b * A;
        float target;
        if (is_double) {
            const float *row = qn_on + b * A;
            const uint8_t *mrow = masked ? mask_next + b * A : nullptr;
            const int a_star = tsm_q_first_argmax(row, mrow, A, mv);
            target = qt[a_star];
        } else {
            target = qt[0];
            for (int a = 1; a < A; ++a) target = fmaxf(target, qt[a]);
        }
        const float ret = tsm_nstep_ret(target, vmask[b] != 0, gpow[b], mc[b]);
        const int64_t ac = act[b];
        const bool ok = ac >= 0 && ac < A;  // an action outside [0, A) reads nothing and poisons the loss
        const float qs = ok ? q[b * A + ac] : __builtin_nanf("");
        const float td = ret - qs;
        float l, g;
        if (huber_delta > 0.f) {
            const float e = -td, ae = fabsf(e);
            l = ae < huber_delta ? 0.5f * e * e : huber_delta * (ae - 0.5f * huber_delta);
            g = (e <= -huber_delta ? -huber_delta : (e >= huber_delta ? huber_delta : e)) / (float)B;
        } else {
            const float wt = weight ? weight[b] : 1.f;
            l = td * td * wt;
            g = -2.f * td * wt / (float)B;
        }
        returns_out[b] = ret;
        td_out[b] = td;
        float *drow = dq + b * A;
        for (int a = 0; a < A; ++a) drow[a] = (ok && a == (int)ac) ? g : 0.f;
        p_l = (double)l;
        p_q = (double)qs;
    }
    p_l = wave_sum(p_l);
    p_q = wave_sum(p_q);
    tsm_store_partials(p_l, p_q, t, lane, w, s_red, partial);
}

// Draws of row r are words of Philox4x32-10 at (seed, counter c + r): the coin is word 0 of tsm_philox4; uniform[a] is word
// a % 4 of the block whose third counter word is 1 + a / 4 (philox.h).
__global__ __launch_bounds__(kDThreads) void dqn_egreedy_kernel(const float *__restrict__ q,
                                                                const uint8_t *__restrict__ mask, int64_t R, int32_t A,
                                                                const float *__restrict__ eps_dev, uint64_t seed,
                                                                uint64_t offset, const uint64_t *__restrict__ offset_dev,
                                                                int32_t *__restrict__ act) {
    const int64_t r = (int64_t)blockIdx.x * kDThreads + threadIdx.x;
    if (r >= R) return;
    const uint64_t c = offset + (offset_dev ? *offset_dev : 0ull) + (uint64_t)r;
    const float eps = *eps_dev;
    const uint8_t *mrow = mask ? mask + r * A : nullptr;
    uint32_t bits[4];
    tsm_philox4(seed, c, bits);
    int a_sel = 0;
    if (tsm_u01(bits[0]) < eps) {  // rand_act = (uniform[A] + mask).argmax()   (dqn.py:166-169)
        float best = 0.f;
        for (int a = 0; a < A; ++a) {
            if ((a & 3) == 0) tsm_philox4_sub(seed, c, 1u + (uint32_t)(a >> 2), bits);
            const float v = tsm_u01(bits[a & 3]) + ((mrow && mrow[a]) ? 1.f : 0.f);
            if (a == 0 || v > best) { best = v; a_sel = a; }
        }
    } else {
        // first argmax of the masked q.  compute_q_value lowers every illegal entry below the smallest logit, so a row with
        // a legal action picks its first best LEGAL entry; a row without one picks the first maximum of the raw row.
        const float *row = q + r * A;
        bool any = false;
        float best = 0.f;
        for (int a = 0; a < A; ++a)
            if (!mrow || mrow[a]) {
                if (!any || row[a] > best) { best = row[a]; a_sel = a; any = true; }
            }
        if (!any)
            for (int a = 0; a < A; ++a)
                if (a == 0 || row[a] > best) { best = row[a]; a_sel = a; }
    }
    act[r] = a_sel;
}

}  // namespace

TSM_EXPORT int tsm_dqn_check(int32_t n_act, int32_t n_step) {
    if (int rc = tsm_q_check_act("tsm_dqn_check", n_act)) return rc;
    TSM_REQUIRE(n_step >= 1, "tsm_dqn_check: n_step_return_horizon should be greater than 0 but got: %d", n_step);
    return TSM_OK;
}

TSM_EXPORT int64_t tsm_dqn_partial_elems(int64_t B) {
    if (B < 1) return -1;
    return 2 * ceil_div(B, kDThreads);
}

TSM_EXPORT int tsm_dqn_td_head(const float *q, const float *q_next_online, const float *q_next_target,
                               const uint8_t *mask_next, const int64_t *act, const float *mc, const float *gpow,
                               const uint8_t *vmask, const float *weight, int64_t B, int32_t n_act, int is_double,
                               float huber_delta, float *returns_out, float *td_error, float *dq, double *partial,
                               void *stream) {
    if (int rc = tsm_q_check_act("tsm_dqn_td_head", n_act)) return rc;
    // (With a mask and is_double every workgroup of 256 rows reads all B * n_act logits for the batch-wide offset: B^2 n_act /
    //  256 loads in all -- 16 MB of L2 reads at B = 4096, n_act = 9, but quadratic in B.  The bound below is the index range,
    //  not a promise of speed: a replay batch far beyond 10^5 masked rows wants a reduction launch of its own.)
    if (int rc = tsm_q_check_rows("tsm_dqn_td_head", B)) return rc;
    TSM_REQUIRE(q && q_next_online && act && mc && gpow && vmask && returns_out && td_error && dq && partial,
                "tsm_dqn_td_head: null pointer");
    hipLaunchKernelGGL(dqn_td_head_kernel, dim3((unsigned)ceil_div(B, kDThreads)), dim3(kDThreads), 0, tsm_stream(stream),
                       q, q_next_online, q_next_target, mask_next, act, mc, gpow, vmask, weight, B, n_act, is_double,
                       huber_delta, returns_out, td_error, dq, partial);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_dqn_egreedy(const float *q, const uint8_t *mask, int64_t R, int32_t n_act, const float *eps_dev,
                               uint64_t seed, uint64_t offset, const uint64_t *offset_dev, int32_t *act_out,
                               void *stream) {
    if (int rc = tsm_q_check_act("tsm_dqn_egreedy", n_act)) return rc;
    TSM_REQUIRE(R >= 0, "tsm_dqn_egreedy: R = %lld is negative", (long long)R);
    if (R == 0) return TSM_OK;
    TSM_REQUIRE(q && eps_dev && act_out, "tsm_dqn_egreedy: null pointer");
    hipLaunchKernelGGL(dqn_egreedy_kernel, dim3((unsigned)ceil_div(R, kDThreads)), dim3(kDThreads), 0, tsm_stream(stream),
                       q, mask, R, n_act, eps_dev, seed, offset, offset_dev, act_out);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}
