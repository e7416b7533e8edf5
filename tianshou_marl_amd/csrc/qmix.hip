// qmix.hip -- QMIX: the monotonic mixer's per-row arithmetic and its backward, the TD head, and epsilon-greedy acting.
//
// Replaces the arithmetic of QMIXMixer.forward (/root/reference/tianshou/algorithm/multiagent/ctde.py:468-499) and of
// QMIXPolicy.learn (:618-702) between the network forwards and `loss.backward()`, and the action choice of
// QMIXPolicy.forward (:557-616) on the device.  The hypernetworks and the agent Q-nets run in csrc/dense.hip.
//
// Per joint row b (E = mixing_embed_dim, N agents):
//   q_i      = Q_i(obs)[b][act_i]                          q'_i = max_a Q'_i(obs_next)[b][a]   (target nets)
//   w1 = |w1raw| [N][E], w2 = |w2raw| [E] (monotonic; else the raw values)
//   pre[e]   = sum_i q_i w1[i][e] + b1[e]                 h[e] = elu(pre[e])
//   q_tot    = sum_e h[e] w2[e] + b2                       q_tot' the same on the target side with q'
//   y        = mean_i rew_i + gamma q_tot' (1 - term_0)    d q_tot = 2 (q_tot - y) / B  (mse_loss over the batch)
// and the backward of the online side (no reduction over rows is needed: every gradient is a function of its row):
//   d b2 = g, d w2raw[e] = g h[e] sgn(w2raw[e]), d pre[e] = g w2[e] (pre > 0 ? 1 : exp(pre)), d b1 = d pre,
//   d w1raw[i][e] = q_i d pre[e] sgn(w1raw[i][e]), d Q_i[b][act_i] = sum_e d pre[e] w1[i][e]   (sgn(0) = 0, as torch.abs)
// Layout: a workgroup owns R consecutive rows; a row is L = E / 4 lanes, each holding 4 mixing units, so the [N][E] /
// [E] rows of the hypernetwork outputs and of their gradients move as 16-B loads / stores, L lanes per 16 L bytes.  The
// per-agent Q rows ([B][A], A small and not 16-B aligned per row) are staged through LDS as the block's contiguous
// R x A segment.  Loss and mean(q_tot) leave as per-workgroup f64 partials; tsm_qmix_finalize sums them in a fixed order.
#include "common.h"
#include "philox.h"

namespace {
constexpr int kQThreads = 256;
constexpr int kQMaxA = 64;
constexpr int kQMaxN = TSM_QMIX_MAX_AGENTS;
constexpr int kGreedyRows = 16;  // rows per workgroup of the epsilon-greedy kernel

struct QPtrs { const float *q[kQMaxN]; };

__device__ __forceinline__ float sgnf(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }
__device__ __forceinline__ float eluf(float x) { return x > 0.f ? x : expm1f(x); }

// src[0, n) -> LDS dst[0, n): consecutive lanes read consecutive addresses, 16 B at a time when src is 16-B aligned
__device__ __forceinline__ void stage_seg(float *dst, const float *__restrict__ src, int n) {
    const int t = threadIdx.x;
    if ((reinterpret_cast<uintptr_t>(src) & 15) == 0) {
        const int n4 = n >> 2;
        for (int i = t; i < n4; i += kQThreads) st4(dst + 4 * i, ld4(src + 4 * i));
        for (int i = 4 * n4 + t; i < n; i += kQThreads) dst[i] = src[i];
    } else {
        for (int i = t; i < n; i += kQThreads) dst[i] = src[i];
    }
}

// sum over the L lanes of a row (an aligned group of L consecutive lanes): xor butterfly, the same bits in every lane
template <int L>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int m = L / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, kWave);
    return v;
}

template <int E>
__global__ __launch_bounds__(kQThreads) void qmix_mix_td_kernel(
    tsm_qmix_agents ag, int32_t N, int32_t A, int64_t B, const float *__restrict__ w1, const float *__restrict__ b1,
    const float *__restrict__ w2, const float *__restrict__ b2, const float *__restrict__ tw1, const float *__restrict__ tb1,
    const float *__restrict__ tw2, const float *__restrict__ tb2, const uint8_t *__restrict__ term, float gamma, int mono,
    float *__restrict__ dw1, float *__restrict__ db1, float *__restrict__ dw2, float *__restrict__ db2,
    double *__restrict__ partial, float *__restrict__ qtot_out) {
    constexpr int L = E / 4;             // lanes per row
    constexpr int RW = kWave / L;        // rows per wave
    constexpr int R = kQThreads / L;     // rows per workgroup
    __shared__ __align__(16) float seg[R * kQMaxA];
    __shared__ float s_qsel[kQMaxN][R], s_qmax[kQMaxN][R], s_dq[kQMaxN][R], s_rew[R], s_g[R], s_qt[R];
    __shared__ int s_act[kQMaxN][R];
    __shared__ double s_red[2][kQThreads / kWave];
    const int t = threadIdx.x;
    const int64_t b0 = (int64_t)blockIdx.x * R;
    const int nr = (int)(B - b0 < R ? B - b0 : R);

    // ---- per agent: target max over the staged [nr][A] segment, the online Q at the taken action ----
    if (t < nr) s_rew[t] = 0.f;
    for (int i = 0; i < N; ++i) {
        stage_seg(seg, ag.q_next[i] + b0 * A, nr * A);
        __syncthreads();
        if (t < nr) {
            const float *row = seg + t * A;
            float m = row[0];
            for (int a = 1; a < A; ++a) m = fmaxf(m, row[a]);
            s_qmax[i][t] = m;
            const int64_t ac = ag.act[i][b0 + t];
            const bool ok = ac >= 0 && ac < A;  // an action outside [0, A) reads nothing and poisons the loss
            s_act[i][t] = ok ? (int)ac : -1;
            s_qsel[i][t] = ok ? ag.q[i][(b0 + t) * A + ac] : __builtin_nanf("");
            s_rew[t] += ag.rew[i][b0 + t];  // torch.stack(rewards, -1).mean(-1): agents in order
        }
        __syncthreads();
    }

    // ---- row phase: L lanes per row, 4 mixing units per lane ----
    const int lane = t & (kWave - 1), g = lane / L, l = lane % L;
    const int r = (t / kWave) * RW + g;
    const bool valid = r < nr;
    const int rr = valid ? r : 0;              // rows past B compute on row b0 and store nothing
    const int64_t b = b0 + rr;
    const int e0 = 4 * l;

    // target side: q_tot'
    float qn;
    {
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int i = 0; i < N; ++i) {
            float4 w = ld4(tw1 + (b * N + i) * E + e0);
            if (mono) w = make_float4(fabsf(w.x), fabsf(w.y), fabsf(w.z), fabsf(w.w));
            const float q = s_qmax[i][rr];
            s.x = fmaf(q, w.x, s.x); s.y = fmaf(q, w.y, s.y); s.z = fmaf(q, w.z, s.z); s.w = fmaf(q, w.w, s.w);
        }
        const float4 bb = ld4(tb1 + b * E + e0);
        float4 v = ld4(tw2 + b * E + e0);
        if (mono) v = make_float4(fabsf(v.x), fabsf(v.y), fabsf(v.z), fabsf(v.w));
        float p = eluf(s.x + bb.x) * v.x;
        p = fmaf(eluf(s.y + bb.y), v.y, p);
        p = fmaf(eluf(s.z + bb.z), v.z, p);
        p = fmaf(eluf(s.w + bb.w), v.w, p);
        qn = group_sum<L>(p) + tb2[b];
    }

    // online side: q_tot and its backward
    float4 wr[kQMaxN];
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int i = 0; i < kQMaxN; ++i) {
        if (i < N) {
            wr[i] = ld4(w1 + (b * N + i) * E + e0);
            const float4 w = mono ? make_float4(fabsf(wr[i].x), fabsf(wr[i].y), fabsf(wr[i].z), fabsf(wr[i].w)) : wr[i];
            const float q = s_qsel[i][rr];
            s.x = fmaf(q, w.x, s.x); s.y = fmaf(q, w.y, s.y); s.z = fmaf(q, w.z, s.z); s.w = fmaf(q, w.w, s.w);
        }
    }
    const float4 bb = ld4(b1 + b * E + e0);
    const float4 pre = make_float4(s.x + bb.x, s.y + bb.y, s.z + bb.z, s.w + bb.w);
    const float4 h = make_float4(eluf(pre.x), eluf(pre.y), eluf(pre.z), eluf(pre.w));
    const float4 v2r = ld4(w2 + b * E + e0);
    const float4 v2 = mono ? make_float4(fabsf(v2r.x), fabsf(v2r.y), fabsf(v2r.z), fabsf(v2r.w)) : v2r;
    float p = h.x * v2.x;
    p = fmaf(h.y, v2.y, p);
    p = fmaf(h.z, v2.z, p);
    p = fmaf(h.w, v2.w, p);
    const float qt = group_sum<L>(p) + b2[b];
    const float y = s_rew[rr] / (float)N + gamma * qn * (term[b] ? 0.f : 1.f);
    const float d = qt - y;
    const float gq = (2.f / (float)B) * d;

    const float4 sg2 = mono ? make_float4(sgnf(v2r.x), sgnf(v2r.y), sgnf(v2r.z), sgnf(v2r.w)) : make_float4(1.f, 1.f, 1.f, 1.f);
    const float4 gw2 = make_float4(h.x * gq * sg2.x, h.y * gq * sg2.y, h.z * gq * sg2.z, h.w * gq * sg2.w);
    const float4 dh = make_float4(gq * v2.x, gq * v2.y, gq * v2.z, gq * v2.w);
    const float4 dp = make_float4(pre.x > 0.f ? dh.x : dh.x * expf(pre.x), pre.y > 0.f ? dh.y : dh.y * expf(pre.y),
                                  pre.z > 0.f ? dh.z : dh.z * expf(pre.z), pre.w > 0.f ? dh.w : dh.w * expf(pre.w));
    if (valid) {
        st4(dw2 + b * E + e0, gw2);
        st4(db1 + b * E + e0, dp);
    }
#pragma unroll
    for (int i = 0; i < kQMaxN; ++i) {
        if (i < N) {
            const float q = s_qsel[i][rr];
            const float4 w = wr[i];
            const float4 sg = mono ? make_float4(sgnf(w.x), sgnf(w.y), sgnf(w.z), sgnf(w.w)) : make_float4(1.f, 1.f, 1.f, 1.f);
            if (valid) st4(dw1 + (b * N + i) * E + e0, make_float4(q * dp.x * sg.x, q * dp.y * sg.y, q * dp.z * sg.z, q * dp.w * sg.w));
            const float4 wa = mono ? make_float4(fabsf(w.x), fabsf(w.y), fabsf(w.z), fabsf(w.w)) : w;
            float dq = dp.x * wa.x;
            dq = fmaf(dp.y, wa.y, dq);
            dq = fmaf(dp.z, wa.z, dq);
            dq = fmaf(dp.w, wa.w, dq);
            dq = group_sum<L>(dq);
            if (valid && l == 0) s_dq[i][r] = dq;
        }
    }
    const bool lead = valid && l == 0;
    if (lead) { s_g[r] = gq; s_qt[r] = qt; }
    double p_sq = lead ? (double)d * (double)d : 0.0, p_q = lead ? (double)qt : 0.0;
    p_sq = wave_sum(p_sq);
    p_q = wave_sum(p_q);
    if (lane == 0) { s_red[0][t / kWave] = p_sq; s_red[1][t / kWave] = p_q; }
    __syncthreads();

    // ---- stores of the block's contiguous segments: d b2 [nr], d Q_i [nr][A] (non-zero only at act) ----
    if (t < nr) {
        db2[b0 + t] = s_g[t];
        if (qtot_out) qtot_out[b0 + t] = s_qt[t];
    }
    for (int i = 0; i < N; ++i) {
        float *dst = ag.dq[i] + b0 * A;
        const int n = nr * A;
        if ((reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
            const int n4 = n >> 2;
            for (int j4 = t; j4 < n4; j4 += kQThreads) {
                float v[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int j = 4 * j4 + k, row = j / A;
                    v[k] = (j - row * A) == s_act[i][row] ? s_dq[i][row] : 0.f;
                }
                st4(dst + 4 * j4, make_float4(v[0], v[1], v[2], v[3]));
            }
            for (int j = 4 * n4 + t; j < n; j += kQThreads) {
                const int row = j / A;
                dst[j] = (j - row * A) == s_act[i][row] ? s_dq[i][row] : 0.f;
            }
        } else {
            for (int j = t; j < n; j += kQThreads) {
                const int row = j / A;
                dst[j] = (j - row * A) == s_act[i][row] ? s_dq[i][row] : 0.f;
            }
        }
    }
    if (t < 2) {
        double acc = 0.0;
        for (int w = 0; w < kQThreads / kWave; ++w) acc += s_red[t][w];
        partial[(int64_t)blockIdx.x * 2 + t] = acc;
    }
}

__global__ __launch_bounds__(kWave) void qmix_finalize_kernel(const double *__restrict__ partial, int32_t nb, int64_t B,
                                                              float *__restrict__ out) {
    // one wave: lane l takes workgroups l, l + 64, ..., then the xor butterfly -- a fixed order
    const int lane = threadIdx.x;
    double s_sq = 0.0, s_q = 0.0;
    for (int i = lane; i < nb; i += kWave) { s_sq += partial[2 * i]; s_q += partial[2 * i + 1]; }
    s_sq = wave_sum(s_sq);
    s_q = wave_sum(s_q);
    if (lane != 0) return;
    out[0] = (float)(s_sq / (double)B);
    out[1] = (float)(s_q / (double)B);
}

__global__ __launch_bounds__(kQThreads) void qmix_egreedy_kernel(QPtrs qp, int32_t N, int32_t A, int64_t B,
                                                                 const float *__restrict__ eps_dev, uint64_t seed,
                                                                 uint64_t offset, const uint64_t *__restrict__ offset_dev,
                                                                 int32_t *__restrict__ act, int64_t stride) {
    __shared__ __align__(16) float sq[kQMaxN * kGreedyRows * kQMaxA];
    const int t = threadIdx.x;
    const int64_t b0 = (int64_t)blockIdx.x * kGreedyRows;
    const int nr = (int)(B - b0 < kGreedyRows ? B - b0 : kGreedyRows);
    for (int i = 0; i < N; ++i) stage_seg(sq + i * kGreedyRows * A, qp.q[i] + b0 * A, nr * A);
    __syncthreads();
    const uint64_t c = offset + (offset_dev ? *offset_dev : 0ull);
    const float eps = *eps_dev;
    // item k = (row, agent) in [E][N] order: with stride == N the stores are consecutive
    for (int k = t; k < nr * N; k += kQThreads) {
        const int rw = k / N, i = k - rw * N;
        const int64_t b = b0 + rw;
        uint32_t bits[4];
        tsm_philox4(seed, c + (uint64_t)i, bits);   // the call's coin for agent i (word 1): shared by every row
        int a;
        if (tsm_u01(bits[1]) < eps) {
            tsm_philox4(seed, c + (uint64_t)b * N + i, bits);  // the row's uniform action (word 0)
            a = (int)(((uint64_t)bits[0] * (uint64_t)A) >> 32);
        } else {
            const float *row = sq + i * kGreedyRows * A + rw * A;
            float m = row[0];
            a = 0;
            for (int j = 1; j < A; ++j)
                if (row[j] > m) { m = row[j]; a = j; }  // first maximum, as torch.argmax
        }
        act[b * stride + i] = a;
    }
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
}  // namespace

TSM_EXPORT int64_t tsm_qmix_partial_elems(int64_t B, int32_t E) {
    if (B < 1 || (E != 32 && E != 64)) return -1;
    return 2 * ceil_div(B, kQThreads / (E / 4));
}

TSM_EXPORT int tsm_qmix_mix_td(const tsm_qmix_agents *agents, int32_t n_agents, int32_t n_act, int64_t B, int32_t E,
                               const float *w1raw, const float *b1, const float *w2raw, const float *b2,
                               const float *tw1raw, const float *tb1, const float *tw2raw, const float *tb2,
                               const uint8_t *term, float gamma, int monotonic, float *dw1, float *db1, float *dw2,
                               float *db2, double *partial, float *qtot_out, void *stream) {
    TSM_REQUIRE(n_agents >= 1 && n_agents <= kQMaxN, "tsm_qmix_mix_td: n_agents = %d outside [1, %d]", n_agents, kQMaxN);
    TSM_REQUIRE(E == 32 || E == 64, "tsm_qmix_mix_td: mixing_embed_dim = %d, must be 32 or 64", E);
    TSM_REQUIRE(n_act >= 1 && n_act <= kQMaxA, "tsm_qmix_mix_td: n_act = %d outside [1, %d]", n_act, kQMaxA);
    TSM_REQUIRE(B >= 1 && B <= ((int64_t)1 << 31) / ((int64_t)n_agents * kQMaxA), "tsm_qmix_mix_td: B = %lld out of range",
                (long long)B);
    TSM_REQUIRE(agents && w1raw && b1 && w2raw && b2 && tw1raw && tb1 && tw2raw && tb2 && term && dw1 && db1 && dw2 && db2
                    && partial, "tsm_qmix_mix_td: null pointer");
    for (int i = 0; i < n_agents; ++i)
        TSM_REQUIRE(agents->q[i] && agents->q_next[i] && agents->act[i] && agents->rew[i] && agents->dq[i],
                    "tsm_qmix_mix_td: null pointer for agent %d", i);
    TSM_REQUIRE(aligned16(w1raw) && aligned16(b1) && aligned16(w2raw) && aligned16(tw1raw) && aligned16(tb1)
                    && aligned16(tw2raw) && aligned16(dw1) && aligned16(db1) && aligned16(dw2),
                "tsm_qmix_mix_td: the [B][N*E] / [B][E] arrays must be 16-byte aligned");
    const int R = kQThreads / (E / 4);
    const unsigned nb = (unsigned)ceil_div(B, R);
    if (E == 32)
        hipLaunchKernelGGL(qmix_mix_td_kernel<32>, dim3(nb), dim3(kQThreads), 0, tsm_stream(stream), *agents, n_agents,
                           n_act, B, w1raw, b1, w2raw, b2, tw1raw, tb1, tw2raw, tb2, term, gamma, monotonic, dw1, db1, dw2,
                           db2, partial, qtot_out);
    else
        hipLaunchKernelGGL(qmix_mix_td_kernel<64>, dim3(nb), dim3(kQThreads), 0, tsm_stream(stream), *agents, n_agents,
                           n_act, B, w1raw, b1, w2raw, b2, tw1raw, tb1, tw2raw, tb2, term, gamma, monotonic, dw1, db1, dw2,
                           db2, partial, qtot_out);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_qmix_finalize(const double *partial, int32_t n_blocks, int64_t B, float *out, void *stream) {
    TSM_REQUIRE(n_blocks >= 1 && B >= 1, "tsm_qmix_finalize: bad sizes");
    TSM_REQUIRE(partial && out, "tsm_qmix_finalize: null pointer");
    hipLaunchKernelGGL(qmix_finalize_kernel, dim3(1), dim3(kWave), 0, tsm_stream(stream), partial, n_blocks, B, out);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_qmix_egreedy(const float *const *q_by_agent_host, int32_t n_agents, int64_t B, int32_t n_act,
                                const float *eps_dev, uint64_t seed, uint64_t offset, const uint64_t *offset_dev,
                                int32_t *act_out, int64_t act_row_stride, void *stream) {
    TSM_REQUIRE(n_agents >= 1 && n_agents <= kQMaxN, "tsm_qmix_egreedy: n_agents = %d outside [1, %d]", n_agents, kQMaxN);
    TSM_REQUIRE(n_act >= 1 && n_act <= kQMaxA, "tsm_qmix_egreedy: n_act = %d outside [1, %d]", n_act, kQMaxA);
    TSM_REQUIRE(B >= 0 && act_row_stride >= n_agents, "tsm_qmix_egreedy: bad sizes (B = %lld, row stride %lld < %d agents)",
                (long long)B, (long long)act_row_stride, n_agents);
    if (B == 0) return TSM_OK;
    TSM_REQUIRE(q_by_agent_host && eps_dev && act_out, "tsm_qmix_egreedy: null pointer");
    QPtrs qp{};
    for (int i = 0; i < n_agents; ++i) {
        TSM_REQUIRE(q_by_agent_host[i], "tsm_qmix_egreedy: null Q array for agent %d", i);
        qp.q[i] = q_by_agent_host[i];
    }
    hipLaunchKernelGGL(qmix_egreedy_kernel, dim3((unsigned)ceil_div(B, kGreedyRows)), dim3(kQThreads), 0, tsm_stream(stream),
                       qp, n_agents, n_act, B, eps_dev, seed, offset, offset_dev, act_out, act_row_stride);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}
