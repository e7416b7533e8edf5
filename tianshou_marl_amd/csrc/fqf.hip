// fqf.hip -- Fully parameterized Quantile Function: the fraction proposal (forward and backward), the fraction-weighted value
// per action and the head that forms the quantile-regression loss, the fraction loss and both gradients.
//
// Replaces FractionProposalNetwork.forward (/root/reference/tianshou/utils/net/discrete.py:240-253) and the backward of
// `fraction_optim.step(...)` through it, the weighted sum of FQFPolicy.forward (fqf.py:94-97), and FQF._target_q after its
// forwards with FQF._update_with_batch between `self.policy(batch)` and the two optimizer steps (fqf.py:178-193, 201-247).
// The embedding at the proposed fractions is csrc/iqn.hip's, the MLPs around it csrc/dense.hip's.
//
// Layouts: a network row is (b, i) = b * N + i, out is [R][N][A] (the reference's [B, A, N] is its transposed view), taus
// [R][N + 1], tau_hats / logp [R][N].  f is the preprocess net's last LINEAR output; g = relu with relu_f, else the identity.
// The products with Wf and with d_logits^T run on v_mfma_f32_16x16x4_f32 (exact f32 products, f32 accumulation in the k order
// of the loop).  Every sum has a fixed order: two runs give the same bits.
#include "common.h"
#include "q_head_dev.h"

namespace {

constexpr int kFThreads = 256;
constexpr int kFWaves = kFThreads / kWave;
constexpr int kFMinN = 3, kFMaxN = 64, kFMaxH = 512;
constexpr int kFRowsPerWave = TSM_IQN_ROWS_PER_BLOCK / kFWaves;
constexpr int kFLd = kFMaxN + 1;   // odd: the 16 rows of a tile start in 16 different banks
static_assert(kFRowsPerWave * kFWaves == TSM_IQN_ROWS_PER_BLOCK, "rows per workgroup");
static_assert(TSM_IQN_ROWS_PER_BLOCK == 16, "one MFMA tile of rows per workgroup");

__device__ __forceinline__ float fqf_g(float v, int relu_f) { return (relu_f && !(v > 0.f)) ? 0.f : v; }

// ---- tsm_fqf_propose -------------------------------------------------------------------------------------------------
// Workgroup = 16 rows; wave w forms the logits of the fractions [16 w, 16 w + 16) of all 16 rows (k = 0 .. H - 1 in order, then
// + bf), leaves them in LDS, and after the barrier owns the rows 4 w .. 4 w + 3 with lane n on fraction n:
//   e[n] = exp(x[n] - max x), se = sum_k e[k], p[n] = e[n] / se, logp[n] = (x[n] - max x) - log(se);
//   taus[0] = 0, taus[n + 1] = taus[n] + p[n];  tau_hats[n] = (taus[n] + taus[n + 1]) / 2;  entropy = -(sum_n p[n] logp[n]);
// every sum over k or n in order.  The logits are f32; from the subtraction of the maximum on, the row's softmax, cumulative sum
// and entropy are carried in f64 and each output is rounded to f32 once.  In f32 the fractions come out a few 1e-7 off, and the
// fraction loss -- second differences of the quantile function between neighbouring fractions -- moves by more than the whole
// float32 forward leaves on it.
__global__ __launch_bounds__(kFThreads) void fqf_propose_kernel(const float *__restrict__ f, const float *__restrict__ Wf,
                                                                const float *__restrict__ bf, int64_t R, int32_t N, int32_t H,
                                                                int relu_f, float *__restrict__ taus,
                                                                float *__restrict__ tau_hats, float *__restrict__ logp,
                                                                float *__restrict__ entropies) {
    __shared__ float s_x[16 * kFLd];
    const int t = threadIdx.x, lane = t & (kWave - 1), w = t / kWave;
    const int64_t m0 = (int64_t)blockIdx.x * 16;
    const int n0 = w * 16;
    if (n0 < N) {   // wave-uniform
        const int64_t ma = m0 + (lane & 15);
        const int nb = n0 + (lane & 15);
        const bool a_ok = ma < R, b_ok = nb < N;
        const float *a_t = f + (a_ok ? ma : 0) * H + (lane >> 4);    // clamped, always-valid addresses + select
        const float *b_t = Wf + (int64_t)(b_ok ? nb : 0) * H + (lane >> 4);
        f4 acc = f4{0.f, 0.f, 0.f, 0.f};
        for (int kk = 0; kk < H; kk += 4) {
            const float a = a_ok ? fqf_g(a_t[kk], relu_f) : 0.f;
            const float b = b_ok ? b_t[kk] : 0.f;
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
        }
        // C fragment: register r of lane l holds [(l >> 4) * 4 + r][l & 15]
        const float bias = b_ok ? bf[nb] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) s_x[((lane >> 4) * 4 + r) * kFLd + nb] = acc[r] + bias;
    }
    __syncthreads();
    const bool in = lane < N;
#pragma unroll
    for (int rr = 0; rr < kFRowsPerWave; ++rr) {
        const int row = w * kFRowsPerWave + rr;
        const int64_t m = m0 + row;
        if (m >= R) break;   // wave-uniform; no barrier follows
        const float *x = s_x + row * kFLd;
        const float xv = in ? x[lane] : -INFINITY;
        const float mx = wave_max(xv);
        // lane n forms e[n] once; every serial sum below walks the lanes k = 0 .. N - 1 in order (k is wave-uniform)
        const double e = in ? exp((double)xv - (double)mx) : 0.0;
        double se = 0.0;
        for (int k = 0; k < N; ++k) se += __shfl(e, k, kWave);
        const double lp = in ? ((double)xv - (double)mx) - log(se) : 0.0;
        const double pv = e / se, plp = pv * lp;
        double cum = 0.0, prev = 0.0, ent = 0.0;
        for (int k = 0; k < N; ++k) {
            const double pk = __shfl(pv, k, kWave);
            if (k <= lane) { prev = cum; cum += pk; }
            ent += __shfl(plp, k, kWave);
        }
        if (in) {
            logp[m * N + lane] = (float)lp;
            taus[m * (N + 1) + lane + 1] = (float)cum;
            tau_hats[m * N + lane] = (float)((prev + cum) / 2.0);
        }
        if (lane == 0) {
            taus[m * (N + 1)] = 0.f;
            entropies[m] = (float)-ent;
        }
    }
}

// ---- tsm_fqf_propose_backward ------------------------------------------------------------------------------------------
// Workgroup (x, z) = 16 feature columns [h0, h0 + 16) x the rows [b0, b1) of slab z.  Wave w owns the fractions
// [16 w, 16 w + 16): dWf[n][h] = sum over the rows, four per MFMA, in row order.  The workgroups x = 0 also fold dbf.
__global__ __launch_bounds__(kFThreads) void fqf_propose_backward_kernel(const float *__restrict__ d_logits,
                                                                         const float *__restrict__ f, int64_t R, int32_t N,
                                                                         int32_t H, int relu_f, int64_t b_per,
                                                                         float *__restrict__ slabs, int64_t slab_stride,
                                                                         int64_t w_off, int64_t b_off) {
    const int t = threadIdx.x, lane = t & (kWave - 1), w = t / kWave;
    const int n0 = w * 16;
    if (n0 >= N) return;   // wave-uniform; no barrier in this kernel
    const int h = blockIdx.x * 16 + (lane & 15);
    const int64_t b0 = (int64_t)blockIdx.y * b_per;
    int64_t b1 = b0 + b_per;
    if (b1 > R) b1 = R;
    float *slab = slabs + (int64_t)blockIdx.y * slab_stride;
    const int n = n0 + (lane & 15);   // this lane's fraction as the A operand
    f4 acc = f4{0.f, 0.f, 0.f, 0.f};
    float bsum = 0.f;
    for (int64_t k0 = b0; k0 < b1; k0 += 4) {
        const int64_t m = k0 + (lane >> 4);
        float a = 0.f, b = 0.f;
        if (m < b1) {
            a = n < N ? d_logits[m * N + n] : 0.f;
            b = fqf_g(f[m * H + h], relu_f);
        }
        bsum += a;
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int nr = n0 + (lane >> 4) * 4 + r;
        if (nr < N) slab[w_off + (int64_t)nr * H + h] = acc[r];
    }
    if (blockIdx.x == 0) {   // rows k0 + 0 .. 3 of fraction n sit in lanes n, n + 16, n + 32, n + 48: folded in that order
        const float s1 = __shfl(bsum, (lane & 15) + 16, kWave), s2 = __shfl(bsum, (lane & 15) + 32, kWave),
                    s3 = __shfl(bsum, (lane & 15) + 48, kWave);
        if (lane < 16 && n < N) slab[b_off + n] = ((bsum + s1) + s2) + s3;
    }
}

// ---- tsm_fqf_values ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kFThreads) void fqf_values_kernel(const float *__restrict__ out, const float *__restrict__ taus,
                                                               int64_t R, int32_t N, int32_t A, float *__restrict__ q) {
    const int64_t g = (int64_t)blockIdx.x * kFThreads + threadIdx.x;
    if (g >= R * A) return;
    const int64_t r = g / A;
    const int a = (int)(g - r * A);
    const float *tr = taus + r * (N + 1);
    float acc = 0.f;
    for (int i = 0; i < N; ++i) acc += (tr[i + 1] - tr[i]) * out[(r * N + i) * A + a];
    q[g] = acc;
}

// ---- tsm_fqf_head ------------------------------------------------------------------------------------------------------
// The launch shape of iqn_head_kernel: one wave per row, kFRowsPerWave rows after one another, 4 waves per workgroup.  Lane i
// holds Qh_i = out[b][i][act] and, for i < N - 1, Q_i = out_tau[b][i][act] with g_{i + 1}.  The quantile part is
// iqn_head_kernel's with n_online = n_target = N, through the same functions of q_head_dev.h.  Fraction part, per row:
//   p_n = expf(logp_n);  taus_k as tsm_fqf_propose wrote them: the fractions at which out_tau was evaluated;
//   fraction loss = sum_k g_k taus_k (xor butterfly over the lanes);  G_m = g_{N - 1} + g_{N - 2} + ... + g_{m + 1} in that
//   order;  Gbar = sum_n p_n G_n (butterfly);  d_logits[m] = (p_m (G_m - Gbar) + ent_coef * (p_m (logp_m + H_b))) / B.
__global__ __launch_bounds__(kFThreads) void fqf_head_kernel(
    const float *__restrict__ out, const float *__restrict__ out_tau, const float *__restrict__ q_next,
    const float *__restrict__ out_next, const uint8_t *__restrict__ mask_next, const float *__restrict__ taus,
    const float *__restrict__ tau_hats, const float *__restrict__ logp, const float *__restrict__ entropies, const int64_t *__restrict__ act,
    const float *__restrict__ mc, const float *__restrict__ gpow, const uint8_t *__restrict__ vmask,
    const float *__restrict__ weight, float ent_coef, int64_t B, int32_t A, int32_t N, float *__restrict__ returns_out,
    float *__restrict__ prio, float *__restrict__ d_out, float *__restrict__ d_logits, double *__restrict__ partial,
    double *__restrict__ partial_frac) {
    __shared__ float s_min[kFWaves], s_max[kFWaves];
    __shared__ float s_ret[kFWaves][kFMaxN], s_d[kFWaves][kFMaxN];
    __shared__ double s_red[2][kFWaves], s_red2[2][kFWaves];
    const int t = threadIdx.x, lane = t & (kWave - 1), w = t / kWave;
    const float mv = mask_next ? tsm_q_mask_offset<kFThreads>(q_next, B * A, s_min, s_max) : 0.f;
    const float nanv = __builtin_nanf("");

    double acc_l = 0.0, acc_q = 0.0, acc_f = 0.0, acc_e = 0.0;
    // every wave walks all its steps (the barriers are workgroup-wide); a row past B only skips its memory traffic
    for (int rr = 0; rr < kFRowsPerWave; ++rr) {
        const int64_t b = (int64_t)blockIdx.x * TSM_IQN_ROWS_PER_BLOCK + w * kFRowsPerWave + rr;
        const bool live = b < B;
        int64_t ac = 0;
        bool ok = false;
        float wt = 1.f, d = 0.f, l_row = 0.f, p_row = 0.f, q_row = 0.f, f_row = 0.f, dl = 0.f;
        if (live) {
            const int a_star = tsm_q_first_argmax(q_next + b * A, mask_next ? mask_next + b * A : nullptr, A, mv);
            const bool vm = vmask[b] != 0;
            const float gp = gpow[b], mcv = mc[b];
            ac = act[b];
            ok = ac >= 0 && ac < A;
            wt = weight ? weight[b] : 1.f;
            if (lane < N) {
                const float ret = tsm_nstep_ret(out_next[(b * N + lane) * A + a_star], vm, gp, mcv);
                returns_out[b * N + lane] = ret;
                s_ret[w][lane] = ret;
            }
        }
        __syncthreads();
        if (live) {
            const bool in = lane < N, inner = lane < N - 1;
            const float c = (in && ok) ? out[(b * N + lane) * A + ac] : 0.f;
            const float tau = in ? tau_hats[b * N + lane] : 0.f;
            tsm_quantile_row(s_ret[w], N, N, lane, c, tau, wt, B, l_row, p_row, q_row, d);
            if (in) s_d[w][lane] = ok ? d : 0.f;
            // the fraction part (fqf.py:227-243): lane i < N - 1 forms g_{i + 1}
            const float qi = (inner && ok) ? out_tau[(b * (N - 1) + lane) * A + ac] : 0.f;
            const float c_up = __shfl_down(c, 1, kWave), q_up = __shfl_down(qi, 1, kWave), q_dn = __shfl_up(qi, 1, kWave);
            const float v1 = qi - c, v2 = qi - c_up;
            const bool sg1 = qi > (lane == 0 ? c : q_dn), sg2 = qi < (lane == N - 2 ? c_up : q_up);
            const float gl = inner ? (sg1 ? v1 : -v1) + (sg2 ? v2 : -v2) : 0.f;
            const float lpm = in ? logp[b * N + lane] : 0.f;
            const float pm = in ? expf(lpm) : 0.f;
            const float tk = inner ? taus[b * (N + 1) + lane + 1] : 0.f;   // the fraction at which Q_i was evaluated
            float G = 0.f;       // G_lane
            for (int i = N - 2; i >= 0; --i) {   // i is wave-uniform: every lane reads lane i's g
                const float gi = __shfl(gl, i, kWave);
                if (i >= lane) G += gi;
            }
            f_row = wave_sum(gl * tk);
            const float gbar = wave_sum(pm * G);
            const float hb = entropies[b];
            dl = (pm * (G - gbar) + ent_coef * (pm * (lpm + hb))) / (float)B;
            if (!ok) l_row = p_row = q_row = f_row = nanv;
            if (in) d_logits[b * N + lane] = ok ? dl : 0.f;
            if (lane == 0) acc_e += (double)hb;
        }
        __syncthreads();
        if (live) {
            tsm_taken_action_scatter(d_out + b * N * A, s_d[w], N, A, ac, ok, lane);
            if (lane == 0) {
                prio[b] = p_row;
                acc_l += (double)l_row;
                acc_q += (double)q_row;
                acc_f += (double)f_row;
            }
        }
        __syncthreads();   // the LDS rows are rewritten by the next row
    }
    tsm_store_partials(acc_l, acc_q, t, lane, w, s_red, partial);
    tsm_store_partials(acc_f, acc_e, t, lane, w, s_red2, partial_frac);
}

int fqf_check(const char *who, int32_t N, int32_t H, int32_t A) {
    TSM_REQUIRE(N >= kFMinN && N <= kFMaxN, "%s: num_fractions = %d outside [%d, %d]", who, N, kFMinN, kFMaxN);
    TSM_REQUIRE(H >= 16 && H <= kFMaxH && H % 16 == 0, "%s: embedding_dim = %d is not a multiple of 16 in [16, %d]", who, H,
                kFMaxH);
    return tsm_q_check_act(who, A);
}
constexpr int64_t kFMaxRows = ((int64_t)1 << 31) / kFMaxH;   // R * H and R * N * A stay far inside 64-bit offsets; grids too
}  // namespace

TSM_EXPORT int tsm_fqf_check(int32_t num_fractions, int32_t embedding_dim, int32_t n_act) {
    return fqf_check("tsm_fqf_check", num_fractions, embedding_dim, n_act);
}

TSM_EXPORT int tsm_fqf_propose(const float *f, const float *Wf, const float *bf, int64_t R, int32_t num_fractions,
                               int32_t embedding_dim, int relu_f, float *taus, float *tau_hats, float *logp, float *entropies,
                               void *stream) {
    if (int rc = fqf_check("tsm_fqf_propose", num_fractions, embedding_dim, 1)) return rc;
    TSM_REQUIRE(R >= 1 && R <= kFMaxRows, "tsm_fqf_propose: R = %lld out of range", (long long)R);
    TSM_REQUIRE(f && Wf && bf && taus && tau_hats && logp && entropies, "tsm_fqf_propose: null pointer");
    hipLaunchKernelGGL(fqf_propose_kernel, dim3((unsigned)ceil_div(R, 16)), dim3(kFThreads), 0, tsm_stream(stream), f, Wf, bf,
                       R, num_fractions, embedding_dim, relu_f, taus, tau_hats, logp, entropies);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_fqf_propose_backward(const float *d_logits, const float *f, int64_t R, int32_t num_fractions,
                                        int32_t embedding_dim, int relu_f, int32_t n_split, float *slabs, int64_t slab_stride,
                                        int64_t w_off, int64_t b_off, void *stream) {
    if (int rc = fqf_check("tsm_fqf_propose_backward", num_fractions, embedding_dim, 1)) return rc;
    TSM_REQUIRE(R >= 1 && R <= kFMaxRows, "tsm_fqf_propose_backward: R = %lld out of range", (long long)R);
    TSM_REQUIRE(n_split >= 1 && n_split <= 65535, "tsm_fqf_propose_backward: n_split = %d out of range", n_split);
    const int64_t nw = (int64_t)num_fractions * embedding_dim;
    TSM_REQUIRE(w_off >= 0 && b_off >= 0 && w_off + nw <= slab_stride && b_off + num_fractions <= slab_stride &&
                    (b_off >= w_off + nw || w_off >= b_off + num_fractions),
                "tsm_fqf_propose_backward: the weight block [%lld, +%lld) and the bias block [%lld, +%d) must lie apart inside "
                "a slab of %lld", (long long)w_off, (long long)nw, (long long)b_off, num_fractions, (long long)slab_stride);
    TSM_REQUIRE(d_logits && f && slabs, "tsm_fqf_propose_backward: null pointer");
    const int64_t b_per = ceil_div(R, n_split);
    dim3 grid((unsigned)(embedding_dim / 16), (unsigned)n_split);
    hipLaunchKernelGGL(fqf_propose_backward_kernel, grid, dim3(kFThreads), 0, tsm_stream(stream), d_logits, f, R,
                       num_fractions, embedding_dim, relu_f, b_per, slabs, slab_stride, w_off, b_off);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_fqf_values(const float *out, const float *taus, int64_t R, int32_t num_fractions, int32_t n_act, float *q,
                              void *stream) {
    if (int rc = fqf_check("tsm_fqf_values", num_fractions, 16, n_act)) return rc;
    TSM_REQUIRE(R >= 0 && R <= kFMaxRows, "tsm_fqf_values: R = %lld out of range", (long long)R);
    if (R == 0) return TSM_OK;
    TSM_REQUIRE(out && taus && q, "tsm_fqf_values: null pointer");
    hipLaunchKernelGGL(fqf_values_kernel, dim3((unsigned)ceil_div(R * n_act, kFThreads)), dim3(kFThreads), 0,
                       tsm_stream(stream), out, taus, R, num_fractions, n_act, q);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_fqf_head(const float *out, const float *out_tau, const float *q_next, const float *out_next,
                            const uint8_t *mask_next, const float *taus, const float *tau_hats, const float *logp,
                            const float *entropies, const int64_t *act, const float *mc, const float *gpow, const uint8_t *vmask, const float *weight,
                            double ent_coef, int64_t B, int32_t n_act, int32_t num_fractions, float *returns_out, float *prio,
                            float *d_out, float *d_logits, double *partial, double *partial_frac, void *stream) {
    if (int rc = fqf_check("tsm_fqf_head", num_fractions, 16, n_act)) return rc;
    if (int rc = tsm_q_check_rows("tsm_fqf_head", B)) return rc;
    TSM_REQUIRE(out && out_tau && q_next && out_next && taus && tau_hats && logp && entropies && act && mc && gpow && vmask &&
                    returns_out && prio && d_out && d_logits && partial && partial_frac,
                "tsm_fqf_head: null pointer");
    hipLaunchKernelGGL(fqf_head_kernel, dim3((unsigned)ceil_div(B, TSM_IQN_ROWS_PER_BLOCK)), dim3(kFThreads), 0,
                       tsm_stream(stream), out, out_tau, q_next, out_next, mask_next, taus, tau_hats, logp, entropies, act, mc,
                       gpow,
                       vmask, weight, (float)ent_coef, B, n_act, num_fractions, returns_out, prio, d_out, d_logits, partial,
                       partial_frac);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}
