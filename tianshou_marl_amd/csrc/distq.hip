// distq.hip -- distributional Q-learning heads: C51 (categorical) and QR-DQN (quantile regression).
//
// Replaces C51Policy.compute_q_value / QRDQNPolicy.compute_q_value (/root/reference/tianshou/algorithm/modelfree/c51.py:66-67,
// qrdqn.py:19-20), C51._target_dist after its forwards with the loss of C51._update_with_batch (c51.py:123-158), and
// QRDQN._target_q after its forwards with QRDQN._update_with_batch (qrdqn.py:94-129), each between the network forwards and
// `optim.step(loss)`.  The Q-network (csrc/dense.hip) emits raw [rows][A * N]; a row is read as [A][N].  The softmax that the
// reference's Net(num_atoms=N, softmax=True) applies inside the module belongs to these kernels.
//
// Shape: one wave per row, kRowsPerWave rows after one another, 4 waves per workgroup.  Atom j of a row lives in lane j % 64,
// register j / 64 (N <= 256: four registers).  Every sum over atoms is a lane-strided partial in register order followed by
// the xor butterfly wave_sum; the N x N tables (the projection of C51, the pairwise Huber terms of QR-DQN) are walked from two
// N-float rows in LDS, k = 0 .. N - 1 in order, and never leave the workgroup.  So two runs give the same bits.
//
// Per row b, both heads:
//   a*      = first argmax_a (q_next[b][a] + (1 - mask[b][a]) * mv), mv over the whole q_next tensor (q_head_dev.h, quirk Q15)
//   nxt[k]  = raw_next[b][a*][k]                      (the lagged net's output when there is one, else the online net's)
//   ret(x)  = (float)((double)(x * vmask) * (double)gpow + (double)mc)           (tsm_nstep_ret, per atom)
// C51:     nd = softmax(nxt);  returns[k] = ret(support[k]);  Tz = clamp(returns, v_min, v_max)
//          m[j] = sum_k clamp(1 - |Tz[k] - z[j]| / dz, 0, 1) nd[k];   p = softmax(raw[b][act]);   ce = -sum_j m[j] log(p[j] + 1e-8)
//          g[j] = -m[j] / (p[j] + 1e-8);   d raw[b][act][k] = p[k] (g[k] - sum_j g[j] p[j]) w / B;   prio = ce;  q = sum p z
// QR-DQN:  returns[j] = ret(nxt[j]);  c = raw[b][act];  u_ij = returns[j] - c[i];  h = smooth_l1(u), beta 1
//          k_ij = |tau_hat[i] - 1[u_ij <= 0]|;   loss_b = (1 / N) sum_i sum_j h_ij k_ij;   prio = (1 / N) sum_i sum_j |h_ij|
//          d c[i] = -(w / (N B)) sum_j k_ij clamp(u_ij, -1, 1);   q = mean_i c[i]
// An action outside [0, A) reads nothing: the row's loss, prio and q are NaN and its gradient zero, as in the DQN head.
// Loss and q leave as per-workgroup f64 partials {sum loss_b w_b, sum q} for tsm_qmix_finalize.
#include "common.h"
#include "q_head_dev.h"

namespace {
constexpr int kZThreads = 256;
constexpr int kZWaves = kZThreads / kWave;
constexpr int kZRowsPerWave = TSM_DISTQ_ROWS_PER_BLOCK / kZWaves;
constexpr int kZMaxN = 256;
constexpr int kZPer = kZMaxN / kWave;
static_assert(kZRowsPerWave * kZWaves == TSM_DISTQ_ROWS_PER_BLOCK, "rows per workgroup");

// softmax over row[0 .. N) as torch: exp(x - max) / sum.  p[i] belongs to atom lane + 64 i (0 past N).
__device__ __forceinline__ void wave_softmax(const float *__restrict__ row, int N, int lane, float p[kZPer]) {
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < kZPer; ++i) {
        const int j = lane + kWave * i;
        p[i] = j < N ? row[j] : -INFINITY;
        mx = fmaxf(mx, p[i]);
    }
    mx = wave_max(mx);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < kZPer; ++i) {
        p[i] = (lane + kWave * i) < N ? expf(p[i] - mx) : 0.f;
        s += p[i];
    }
    s = wave_sum(s);
#pragma unroll
    for (int i = 0; i < kZPer; ++i) p[i] = p[i] / s;
}

__global__ __launch_bounds__(kZThreads) void distq_values_kernel(const float *__restrict__ raw,
                                                                 const float *__restrict__ support, int64_t R, int32_t A,
                                                                 int32_t N, float *__restrict__ q,
                                                                 float *__restrict__ probs) {
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    float z[kZPer];
#pragma unroll
    for (int i = 0; i < kZPer; ++i) z[i] = (support && lane + kWave * i < N) ? support[lane + kWave * i] : 0.f;
    for (int rr = 0; rr < kZRowsPerWave; ++rr) {
        const int64_t r = (int64_t)blockIdx.x * TSM_DISTQ_ROWS_PER_BLOCK + w * kZRowsPerWave + rr;
        if (r >= R) return;
        for (int a = 0; a < A; ++a) {
            const float *row = raw + (r * A + a) * N;
            float p[kZPer], s = 0.f;
            if (support) {
                wave_softmax(row, N, lane, p);
#pragma unroll
                for (int i = 0; i < kZPer; ++i) {
                    s += p[i] * z[i];
                    if (probs && lane + kWave * i < N) probs[(r * A + a) * N + lane + kWave * i] = p[i];
                }
                s = wave_sum(s);
            } else {
#pragma unroll
                for (int i = 0; i < kZPer; ++i) s += (lane + kWave * i) < N ? row[lane + kWave * i] : 0.f;
                s = wave_sum(s) / (float)N;
            }
            if (lane == 0) q[r * A + a] = s;
        }
    }
}

// The two heads share everything but the per-row arithmetic: the offset, a*, the walk over the workgroup's rows and the
// partials.  CAT: C51 (aux = support); else QR-DQN (aux = tau_hat).
template <bool CAT>
__global__ __launch_bounds__(kZThreads) void distq_head_kernel(
    const float *__restrict__ raw, const float *__restrict__ q_next, const float *__restrict__ raw_next,
    const uint8_t *__restrict__ mask_next, const int64_t *__restrict__ act, const float *__restrict__ mc,
    const float *__restrict__ gpow, const uint8_t *__restrict__ vmask, const float *__restrict__ weight,
    const float *__restrict__ aux, int64_t B, int32_t A, int32_t N, float v_min, float v_max, float dz,
    float *__restrict__ returns_out, float *__restrict__ prio, float *__restrict__ d_out, double *__restrict__ partial) {
    __shared__ float s_min[kZWaves], s_max[kZWaves];
    __shared__ float s_a[kZWaves][kZMaxN], s_b[kZWaves][kZMaxN];
    __shared__ double s_red[2][kZWaves];
    const int t = threadIdx.x, lane = t & (kWave - 1), w = t / kWave;
    const float mv = mask_next ? tsm_q_mask_offset<kZThreads>(q_next, B * A, s_min, s_max) : 0.f;
    const float nanv = __builtin_nanf("");

    float x[kZPer];   // support (C51) or tau_hat (QR-DQN) of this lane's atoms
#pragma unroll
    for (int i = 0; i < kZPer; ++i) x[i] = (lane + kWave * i) < N ? aux[lane + kWave * i] : 0.f;

    double acc_l = 0.0, acc_q = 0.0;
    // every wave walks all kZRowsPerWave steps (the barriers are workgroup-wide); a row past B only skips its memory traffic
    for (int rr = 0; rr < kZRowsPerWave; ++rr) {
        const int64_t b = (int64_t)blockIdx.x * TSM_DISTQ_ROWS_PER_BLOCK + w * kZRowsPerWave + rr;
        const bool live = b < B;
        int64_t ac = 0;
        bool ok = false, vm = false;
        float gp = 0.f, mcv = 0.f, wt = 1.f;
        if (live) {
            const int a_star = tsm_q_first_argmax(q_next + b * A, mask_next ? mask_next + b * A : nullptr, A, mv);
            const float *nrow = raw_next + (b * A + a_star) * N;
            ac = act[b];
            ok = ac >= 0 && ac < A;
            vm = vmask[b] != 0;
            gp = gpow[b];
            mcv = mc[b];
            wt = weight ? weight[b] : 1.f;
            if constexpr (CAT) {
                float nd[kZPer];
                wave_softmax(nrow, N, lane, nd);
#pragma unroll
                for (int i = 0; i < kZPer; ++i) {
                    const int j = lane + kWave * i;
                    if (j < N) {
                        const float ret = tsm_nstep_ret(x[i], vm, gp, mcv);
                        returns_out[b * N + j] = ret;
                        s_a[w][j] = ret != ret ? ret : fminf(fmaxf(ret, v_min), v_max);   // clamp keeps a NaN
                        s_b[w][j] = nd[i];
                    }
                }
            } else {
#pragma unroll
                for (int i = 0; i < kZPer; ++i) {
                    const int j = lane + kWave * i;
                    if (j < N) {
                        const float ret = tsm_nstep_ret(nrow[j], vm, gp, mcv);
                        returns_out[b * N + j] = ret;
                        s_a[w][j] = ret;
                    }
                }
            }
        }
        __syncthreads();
        if (live) {
            const float *crow = raw + (b * A + (ok ? ac : 0)) * N;
            float d[kZPer], l_row, p_row, q_row;
            if constexpr (CAT) {
                float m[kZPer] = {0.f, 0.f, 0.f, 0.f};
                for (int k = 0; k < N; ++k) {
                    const float tz = s_a[w][k], ndk = s_b[w][k];
#pragma unroll
                    for (int i = 0; i < kZPer; ++i) {
                        const float c = 1.f - fabsf(tz - x[i]) / dz;
                        m[i] += (c != c ? c : fminf(fmaxf(c, 0.f), 1.f)) * ndk;
                    }
                }
                float p[kZPer], ce = 0.f, gp_sum = 0.f, ev = 0.f, g[kZPer];
                wave_softmax(crow, N, lane, p);
#pragma unroll
                for (int i = 0; i < kZPer; ++i) {
                    const bool in = (lane + kWave * i) < N;
                    const float pe = p[i] + 1e-8f;
                    ce += in ? m[i] * logf(pe) : 0.f;
                    g[i] = in ? -m[i] / pe : 0.f;
                    gp_sum += g[i] * p[i];
                    ev += p[i] * x[i];
                }
                ce = -wave_sum(ce);
                gp_sum = wave_sum(gp_sum);
                ev = wave_sum(ev);
#pragma unroll
                for (int i = 0; i < kZPer; ++i) d[i] = p[i] * (g[i] - gp_sum) * wt / (float)B;
                l_row = ce * wt;
                p_row = ce;
                q_row = ev;
            } else {
                float c[kZPer], ls[kZPer] = {0.f, 0.f, 0.f, 0.f}, ps[kZPer] = {0.f, 0.f, 0.f, 0.f},
                                gs[kZPer] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int i = 0; i < kZPer; ++i) c[i] = (lane + kWave * i) < N ? crow[lane + kWave * i] : 0.f;
                for (int k = 0; k < N; ++k) {
                    const float tk = s_a[w][k];
#pragma unroll
                    for (int i = 0; i < kZPer; ++i) tsm_quantile_huber(tk - c[i], x[i], ls[i], ps[i], gs[i]);
                }
                float l = 0.f, pr = 0.f, cm = 0.f;
#pragma unroll
                for (int i = 0; i < kZPer; ++i) {
                    const bool in = (lane + kWave * i) < N;
                    l += in ? ls[i] : 0.f;
                    pr += in ? ps[i] : 0.f;
                    cm += c[i];
                    d[i] = -(wt / ((float)N * (float)B)) * gs[i];
                }
                l = wave_sum(l) / (float)N;
                p_row = wave_sum(pr) / (float)N;
                q_row = wave_sum(cm) / (float)N;
                l_row = l * wt;
            }
            if (!ok) l_row = p_row = q_row = nanv;
            // the gradient: zero in every other action's slots (and in all of a poisoned row's)
            float *drow = d_out + b * A * N;
            const int lo = ok ? (int)ac * N : -1, hi = lo + N;
            for (int e = lane; e < A * N; e += kWave)
                if (!ok || e < lo || e >= hi) drow[e] = 0.f;
            if (ok) {
#pragma unroll
                for (int i = 0; i < kZPer; ++i)
                    if (lane + kWave * i < N) drow[lo + lane + kWave * i] = d[i];
            }
            if (lane == 0) {
                prio[b] = p_row;
                acc_l += (double)l_row;
                acc_q += (double)q_row;
            }
        }
        __syncthreads();   // the LDS rows are rewritten by the next row
    }
    tsm_store_partials(acc_l, acc_q, t, lane, w, s_red, partial);
}

int distq_check(const char *who, int32_t A, int32_t N) {
    if (int rc = tsm_q_check_act(who, A)) return rc;
    TSM_REQUIRE(N >= 2 && N <= kZMaxN, "%s: n_atoms = %d outside [2, %d]", who, N, kZMaxN);
    return TSM_OK;
}

template <bool CAT>
int distq_head(const char *who, const float *raw, const float *q_next, const float *raw_next, const uint8_t *mask_next,
               const int64_t *act, const float *mc, const float *gpow, const uint8_t *vmask, const float *weight,
               const float *aux, int64_t B, int32_t A, int32_t N, double v_min, double v_max, float *returns_out, float *prio,
               float *d_out, double *partial, void *stream) {
    if (int rc = distq_check(who, A, N)) return rc;
    if (int rc = tsm_q_check_rows(who, B)) return rc;   // B * A * N stays below 2^31 * 256: the row offsets are 64-bit
    if (CAT) TSM_REQUIRE(v_min < v_max, "%s: v_max should be larger than v_min, but got v_min=%g and v_max=%g", who, v_min, v_max);
    TSM_REQUIRE(raw && q_next && raw_next && act && mc && gpow && vmask && aux && returns_out && prio && d_out && partial,
                "%s: null pointer", who);
    const float dz = CAT ? (float)((v_max - v_min) / (double)(N - 1)) : 0.f;
    hipLaunchKernelGGL(distq_head_kernel<CAT>, dim3((unsigned)ceil_div(B, TSM_DISTQ_ROWS_PER_BLOCK)), dim3(kZThreads), 0,
                       tsm_stream(stream), raw, q_next, raw_next, mask_next, act, mc, gpow, vmask, weight, aux, B, A, N,
                       (float)v_min, (float)v_max, dz, returns_out, prio, d_out, partial);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}
}  // namespace

TSM_EXPORT int tsm_distq_check(int32_t n_act, int32_t n_atoms) { return distq_check("tsm_distq_check", n_act, n_atoms); }

TSM_EXPORT int tsm_distq_values(const float *raw, const float *support, int64_t R, int32_t n_act, int32_t n_atoms,
                                int categorical, float *q, float *probs, void *stream) {
    if (int rc = distq_check("tsm_distq_values", n_act, n_atoms)) return rc;
    TSM_REQUIRE(R >= 0 && R <= ((int64_t)1 << 31) / kQHeadMaxA, "tsm_distq_values: R = %lld out of range", (long long)R);
    TSM_REQUIRE(categorical || !probs, "tsm_distq_values: probabilities belong to the categorical mode");
    if (R == 0) return TSM_OK;
    TSM_REQUIRE(raw && q && (!categorical || support), "tsm_distq_values: null pointer");
    hipLaunchKernelGGL(distq_values_kernel, dim3((unsigned)ceil_div(R, TSM_DISTQ_ROWS_PER_BLOCK)), dim3(kZThreads), 0,
                       tsm_stream(stream), raw, categorical ? support : nullptr, R, n_act, n_atoms, q, probs);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_c51_head(const float *raw, const float *q_next, const float *raw_next, const uint8_t *mask_next,
                            const int64_t *act, const float *mc, const float *gpow, const uint8_t *vmask,
                            const float *weight, const float *support, int64_t B, int32_t n_act, int32_t n_atoms,
                            double v_min, double v_max, float *returns_out, float *prio, float *d_out, double *partial,
                            void *stream) {
    return distq_head<true>("tsm_c51_head", raw, q_next, raw_next, mask_next, act, mc, gpow, vmask, weight, support, B, n_act,
                            n_atoms, v_min, v_max, returns_out, prio, d_out, partial, stream);
}

TSM_EXPORT int tsm_qrdqn_head(const float *raw, const float *q_next, const float *raw_next, const uint8_t *mask_next,
                              const int64_t *act, const float *mc, const float *gpow, const uint8_t *vmask,
                              const float *weight, const float *tau_hat, int64_t B, int32_t n_act, int32_t n_quantiles,
                              float *returns_out, float *prio, float *d_out, double *partial, void *stream) {
    return distq_head<false>("tsm_qrdqn_head", raw, q_next, raw_next, mask_next, act, mc, gpow, vmask, weight, tau_hat, B,
                             n_act, n_quantiles, 0.0, 0.0, returns_out, prio, d_out, partial, stream);
}
