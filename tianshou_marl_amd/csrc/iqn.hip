// iqn.hip -- Implicit Quantile Network: the fraction draw, the cosine embedding (forward and backward), the value per action
// and the quantile-regression head over per-row fractions.
//
// Replaces `torch.rand` and CosineEmbeddingNetwork.forward with the product of ImplicitQuantileNetwork.forward
// (/root/reference/tianshou/utils/net/discrete.py:145-161, 208-216) and `loss.backward()` through them,
// QRDQNPolicy.compute_q_value on the [B, A, S] view (qrdqn.py:19-20), and QRDQN._target_q after its forwards with
// IQN._update_with_batch between `self.policy(batch)` and `optim.step(loss)` (qrdqn.py:94-106, iqn.py:160-181).  The two MLPs
// around the embedding (`preprocess`, `last`) run in csrc/dense.hip.
//
// Layouts: a network row is (b, s) = b * S + s, so out is [R][S][A] (sample-major: the reference's [B, A, S] is its transposed
// view), e and phi are [R * S][H], taus [R][S].
//   c[b,s,i]  = cosf(tau[b,s] * (f32(pi) * f32(i))), i = 1 .. C: both products rounded to f32, no fma (-ffp-contract=off)
//   phi[b,s]  = relu(We c[b,s] + be);   e[b,s] = g(f[b]) * phi[b,s], g = relu when the preprocess net ends in its activation
//   (the reference's Net does), else the identity; f is always the value BEFORE g
// The products with We run on v_mfma_f32_16x16x4_f32 (exact f32 products, f32 accumulation in the k order of the loop), the
// cosines are formed in LDS (forward) or registers (backward) and never reach HBM.  Every sum has a fixed order: two runs give
// the same bits.
#include "common.h"
#include "philox.h"
#include "q_head_dev.h"

namespace {

constexpr int kIThreads = 256;
constexpr int kIWaves = kIThreads / kWave;
constexpr int kIMaxS = 64, kIMaxC = 64, kIMaxH = 512;
constexpr int kIRowsPerWave = TSM_IQN_ROWS_PER_BLOCK / kIWaves;
constexpr int kCosLd = kIMaxC + 2;   // 2 x odd: the operand reads [lane & 15][k + (lane >> 4)] meet no bank twice
constexpr uint64_t kTauKey = 0x5355415451495F4Eull;   // folded into the seed: a Philox key no epsilon draw uses
static_assert(kIRowsPerWave * kIWaves == TSM_IQN_ROWS_PER_BLOCK, "rows per workgroup");

__device__ __forceinline__ float iqn_cos(float tau, int i) {
    const float i_pi = 3.14159265358979323846f * (float)i;
    const float arg = tau * i_pi;
    return cosf(arg);
}

// ---- tsm_iqn_taus ---------------------------------------------------------------------------------------------------
// Row r draws at Philox counter c + r under the key seed ^ kTauKey; fraction s is word s % 4 of block s / 4 (philox.h).
__global__ __launch_bounds__(kIThreads) void iqn_taus_kernel(int64_t R, int32_t S, uint64_t seed, uint64_t offset,
                                                             const uint64_t *__restrict__ offset_dev,
                                                             float *__restrict__ taus) {
    const int64_t g = (int64_t)blockIdx.x * kIThreads + threadIdx.x;   // one thread per group of four fractions
    const int per = (S + 3) / 4;
    if (g >= R * per) return;
    const int64_t r = g / per;
    const int q = (int)(g - r * per);
    const uint64_t counter = offset + (offset_dev ? *offset_dev : 0ull) + (uint64_t)r;
    uint32_t bits[4];
    tsm_philox4_sub(seed ^ kTauKey, counter, (uint32_t)q, bits);
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (q * 4 + j < S) taus[r * S + q * 4 + j] = tsm_u01(bits[j]);
}

// ---- tsm_iqn_embed_forward -------------------------------------------------------------------------------------------
// Workgroup = 16 network rows x 64 embedding columns; wave w owns columns [n0 + 16 w, n0 + 16 w + 16).
__global__ __launch_bounds__(kIThreads) void iqn_embed_forward_kernel(const float *__restrict__ f,
                                                                      const float *__restrict__ taus,
                                                                      const float *__restrict__ We,
                                                                      const float *__restrict__ be, int64_t M, int32_t S,
                                                                      int32_t C, int32_t H, int relu_f, float *__restrict__ e,
                                                                      float *__restrict__ phi) {
    __shared__ float s_cos[16 * kCosLd];
    const int t = threadIdx.x, lane = t & (kWave - 1), w = t / kWave;
    const int64_t m0 = (int64_t)blockIdx.y * 16;
    const int n0 = blockIdx.x * 64 + w * 16;
    for (int idx = t; idx < 16 * C; idx += kIThreads) {
        const int r = idx / C, i = idx - r * C;
        const int64_t m = m0 + r;
        s_cos[r * kCosLd + i] = m < M ? iqn_cos(taus[m], i + 1) : 0.f;   // taus [R][S] flat is indexed by the network row
    }
    __syncthreads();
    if (n0 >= H) return;   // wave-uniform; no barrier follows (H is a multiple of 16: a wave's columns are all in or all out)
    f4 acc = f4{0.f, 0.f, 0.f, 0.f};
    const float *a_t = s_cos + (lane & 15) * kCosLd + (lane >> 4);
    const float *b_t = We + (int64_t)(n0 + (lane & 15)) * C + (lane >> 4);
    for (int kk = 0; kk < C; kk += 4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a_t[kk], b_t[kk], acc, 0, 0, 0);
    // C fragment: register r of lane l holds [(l >> 4) * 4 + r][l & 15]
    const int col = n0 + (lane & 15);
    const float bias = be[col];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t m = m0 + (lane >> 4) * 4 + r;
        if (m >= M) continue;
        const float v = acc[r] + bias;
        const float p = v > 0.f ? v : 0.f;
        phi[m * H + col] = p;
        const float fr = f[(m / S) * H + col];
        e[m * H + col] = ((relu_f && !(fr > 0.f)) ? 0.f : fr) * p;
    }
}

// ---- tsm_iqn_embed_backward ------------------------------------------------------------------------------------------
// Workgroup (x, z) = 16 embedding columns [h0, h0 + 16) x the batch rows [b0, b1) of slab z, all S samples of each.  Wave w
// owns the cosines [16 w, 16 w + 16): dWe[h][c] = sum over the network rows, four per MFMA, in row order.  Wave 0 also folds
// dbe.  Then every thread forms d_f for the workgroup's rows and columns, s in order.
__global__ __launch_bounds__(kIThreads) void iqn_embed_backward_kernel(
    const float *__restrict__ d_e, const float *__restrict__ f, const float *__restrict__ phi,
    const float *__restrict__ taus, int64_t R, int32_t S, int32_t C, int32_t H, int relu_f, int64_t b_per, float *__restrict__ d_f,
    float *__restrict__ slabs, int64_t slab_stride, int64_t w_off, int64_t b_off) {
    const int t = threadIdx.x, lane = t & (kWave - 1), w = t / kWave;
    const int h0 = blockIdx.x * 16;
    const int64_t b0 = (int64_t)blockIdx.y * b_per;
    int64_t b1 = b0 + b_per;
    if (b1 > R) b1 = R;
    const int64_t mbeg = b0 * S, mend = b1 > b0 ? b1 * S : mbeg;
    float *slab = slabs + (int64_t)blockIdx.y * slab_stride;

    if (w * 16 < C) {   // wave-uniform; no barrier in this kernel
        f4 acc = f4{0.f, 0.f, 0.f, 0.f};
        float bsum = 0.f;
        const int h = h0 + (lane & 15);
        const int ci = w * 16 + (lane & 15);   // this lane's cosine as the B operand
        for (int64_t k0 = mbeg; k0 < mend; k0 += 4) {
            const int64_t m = k0 + (lane >> 4);
            float a = 0.f, c = 0.f;
            if (m < mend) {
                const float p = phi[m * H + h];
                const float fr = f[(m / S) * H + h];
                a = (p > 0.f && !(relu_f && !(fr > 0.f))) ? d_e[m * H + h] * fr : 0.f;
                c = ci < C ? iqn_cos(taus[m], ci + 1) : 0.f;
            }
            bsum += a;
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, c, acc, 0, 0, 0);
        }
        const int cc = w * 16 + (lane & 15);
        if (cc < C) {
#pragma unroll
            for (int r = 0; r < 4; ++r) slab[w_off + (int64_t)(h0 + (lane >> 4) * 4 + r) * C + cc] = acc[r];
        }
        if (w == 0) {   // rows k0 + 0 .. 3 of column h sit in lanes h, h + 16, h + 32, h + 48: folded in that order
            const float s1 = __shfl(bsum, (lane & 15) + 16, kWave), s2 = __shfl(bsum, (lane & 15) + 32, kWave),
                        s3 = __shfl(bsum, (lane & 15) + 48, kWave);
            if (lane < 16) slab[b_off + h] = ((bsum + s1) + s2) + s3;
        }
    }
    const int hh = h0 + (t & 15);
    for (int64_t b = b0 + (t >> 4); b < b1; b += kIThreads / 16) {
        float acc = 0.f;
        for (int s = 0; s < S; ++s) {
            const int64_t m = b * S + s;
            acc += d_e[m * H + hh] * phi[m * H + hh];
        }
        d_f[b * H + hh] = (relu_f && !(f[b * H + hh] > 0.f)) ? 0.f : acc;
    }
}

// ---- tsm_iqn_values --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kIThreads) void iqn_values_kernel(const float *__restrict__ out, int64_t R, int32_t S, int32_t A,
                                                               float *__restrict__ q) {
    const int64_t g = (int64_t)blockIdx.x * kIThreads + threadIdx.x;
    if (g >= R * A) return;
    const int64_t r = g / A;
    const int a = (int)(g - r * A);
    float acc = 0.f;
    for (int s = 0; s < S; ++s) acc += out[(r * S + s) * A + a];
    q[g] = acc / (float)S;
}

// ---- tsm_iqn_head ----------------------------------------------------------------------------------------------------
// One wave per row, kIRowsPerWave rows after one another, 4 waves per workgroup (the shape of distq_head_kernel<false>).  Lane
// i holds online sample i; the N' targets of the row sit in LDS and are walked j = 0 .. N' - 1 in order.
__global__ __launch_bounds__(kIThreads) void iqn_head_kernel(
    const float *__restrict__ out, const float *__restrict__ q_next, const float *__restrict__ out_next,
    const uint8_t *__restrict__ mask_next, const float *__restrict__ taus, const int64_t *__restrict__ act,
    const float *__restrict__ mc, const float *__restrict__ gpow, const uint8_t *__restrict__ vmask,
    const float *__restrict__ weight, int64_t B, int32_t A, int32_t N, int32_t Np, float *__restrict__ returns_out,
    float *__restrict__ prio, float *__restrict__ d_out, double *__restrict__ partial) {
    __shared__ float s_min[kIWaves], s_max[kIWaves];
    __shared__ float s_ret[kIWaves][kIMaxS], s_d[kIWaves][kIMaxS];
    __shared__ double s_red[2][kIWaves];
    const int t = threadIdx.x, lane = t & (kWave - 1), w = t / kWave;
    const float mv = mask_next ? tsm_q_mask_offset<kIThreads>(q_next, B * A, s_min, s_max) : 0.f;
    const float nanv = __builtin_nanf("");

    double acc_l = 0.0, acc_q = 0.0;
    // every wave walks all its steps (the barriers are workgroup-wide); a row past B only skips its memory traffic
    for (int rr = 0; rr < kIRowsPerWave; ++rr) {
        const int64_t b = (int64_t)blockIdx.x * TSM_IQN_ROWS_PER_BLOCK + w * kIRowsPerWave + rr;
        const bool live = b < B;
        int64_t ac = 0;
        bool ok = false;
        float wt = 1.f, d = 0.f, l_row = 0.f, p_row = 0.f, q_row = 0.f;
        if (live) {
            const int a_star = tsm_q_first_argmax(q_next + b * A, mask_next ? mask_next + b * A : nullptr, A, mv);
            const bool vm = vmask[b] != 0;
            const float gp = gpow[b], mcv = mc[b];
            ac = act[b];
            ok = ac >= 0 && ac < A;
            wt = weight ? weight[b] : 1.f;
            if (lane < Np) {
                const float ret = tsm_nstep_ret(out_next[(b * Np + lane) * A + a_star], vm, gp, mcv);
                returns_out[b * Np + lane] = ret;
                s_ret[w][lane] = ret;
            }
        }
        __syncthreads();
        if (live) {
            const bool in = lane < N;
            const float c = (in && ok) ? out[(b * N + lane) * A + ac] : 0.f;
            const float tau = in ? taus[b * N + lane] : 0.f;
            tsm_quantile_row(s_ret[w], Np, N, lane, c, tau, wt, B, l_row, p_row, q_row, d);
            if (!ok) l_row = p_row = q_row = nanv;
            if (in) s_d[w][lane] = ok ? d : 0.f;
        }
        __syncthreads();
        if (live) {
            tsm_taken_action_scatter(d_out + b * N * A, s_d[w], N, A, ac, ok, lane);
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

int iqn_check(const char *who, int32_t C, int32_t H, int32_t S, int32_t A) {
    TSM_REQUIRE(C >= 4 && C <= kIMaxC && C % 4 == 0, "%s: num_cosines = %d is not a multiple of 4 in [4, %d]", who, C, kIMaxC);
    TSM_REQUIRE(H >= 16 && H <= kIMaxH && H % 16 == 0, "%s: embedding_dim = %d is not a multiple of 16 in [16, %d]", who, H,
                kIMaxH);
    TSM_REQUIRE(S >= 2 && S <= kIMaxS, "%s: sample_size = %d outside [2, %d]", who, S, kIMaxS);
    return tsm_q_check_act(who, A);
}
constexpr int64_t kIMaxRows = ((int64_t)1 << 31) / kIMaxH;   // R * S * H stays inside 64-bit offsets with room; grid.y too
}  // namespace

TSM_EXPORT int tsm_iqn_check(int32_t num_cosines, int32_t embedding_dim, int32_t sample_size, int32_t n_act) {
    return iqn_check("tsm_iqn_check", num_cosines, embedding_dim, sample_size, n_act);
}

TSM_EXPORT int tsm_iqn_taus(int64_t R, int32_t sample_size, uint64_t seed, uint64_t offset, const uint64_t *offset_dev,
                            float *taus, void *stream) {
    TSM_REQUIRE(sample_size >= 2 && sample_size <= kIMaxS, "tsm_iqn_taus: sample_size = %d outside [2, %d]", sample_size,
                kIMaxS);
    TSM_REQUIRE(R >= 0 && R <= kIMaxRows, "tsm_iqn_taus: R = %lld out of range", (long long)R);
    if (R == 0) return TSM_OK;
    TSM_REQUIRE(taus, "tsm_iqn_taus: null pointer");
    const int64_t n = R * ((sample_size + 3) / 4);
    hipLaunchKernelGGL(iqn_taus_kernel, dim3((unsigned)ceil_div(n, kIThreads)), dim3(kIThreads), 0, tsm_stream(stream), R,
                       sample_size, seed, offset, offset_dev, taus);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_iqn_embed_forward(const float *f, const float *taus, const float *We, const float *be, int64_t R,
                                     int32_t sample_size, int32_t num_cosines, int32_t embedding_dim, int relu_f, float *e,
                                     float *phi, void *stream) {
    if (int rc = iqn_check("tsm_iqn_embed_forward", num_cosines, embedding_dim, sample_size, 1)) return rc;
    TSM_REQUIRE(R >= 1 && R * sample_size <= kIMaxRows, "tsm_iqn_embed_forward: R = %lld out of range", (long long)R);
    TSM_REQUIRE(f && taus && We && be && e && phi, "tsm_iqn_embed_forward: null pointer");
    const int64_t M = R * sample_size;
    TSM_REQUIRE(ceil_div(M, 16) <= 65535, "tsm_iqn_embed_forward: %lld network rows are too many for one launch (max %d)",
                (long long)M, 65535 * 16);
    dim3 grid((unsigned)ceil_div(embedding_dim, 64), (unsigned)ceil_div(M, 16));
    hipLaunchKernelGGL(iqn_embed_forward_kernel, grid, dim3(kIThreads), 0, tsm_stream(stream), f, taus, We, be, M, sample_size,
                       num_cosines, embedding_dim, relu_f, e, phi);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_iqn_embed_backward(const float *d_e, const float *f, const float *phi, const float *taus, int64_t R,
                                      int32_t sample_size, int32_t num_cosines, int32_t embedding_dim, int relu_f,
                                      float *d_f, int32_t n_split, float *slabs, int64_t slab_stride, int64_t w_off, int64_t b_off,
                                      void *stream) {
    if (int rc = iqn_check("tsm_iqn_embed_backward", num_cosines, embedding_dim, sample_size, 1)) return rc;
    TSM_REQUIRE(R >= 1 && R * sample_size <= kIMaxRows, "tsm_iqn_embed_backward: R = %lld out of range", (long long)R);
    TSM_REQUIRE(n_split >= 1 && n_split <= 65535, "tsm_iqn_embed_backward: n_split = %d out of range", n_split);
    const int64_t nw = (int64_t)embedding_dim * num_cosines;
    TSM_REQUIRE(w_off >= 0 && b_off >= 0 && w_off + nw <= slab_stride && b_off + embedding_dim <= slab_stride &&
                    (b_off >= w_off + nw || w_off >= b_off + embedding_dim),
                "tsm_iqn_embed_backward: the weight block [%lld, +%lld) and the bias block [%lld, +%d) must lie apart inside a "
                "slab of %lld", (long long)w_off, (long long)nw, (long long)b_off, embedding_dim, (long long)slab_stride);
    TSM_REQUIRE(d_e && f && phi && taus && d_f && slabs, "tsm_iqn_embed_backward: null pointer");
    const int64_t b_per = ceil_div(R, n_split);
    dim3 grid((unsigned)(embedding_dim / 16), (unsigned)n_split);
    hipLaunchKernelGGL(iqn_embed_backward_kernel, grid, dim3(kIThreads), 0, tsm_stream(stream), d_e, f, phi, taus, R,
                       sample_size, num_cosines, embedding_dim, relu_f, b_per, d_f, slabs, slab_stride, w_off, b_off);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_iqn_values(const float *out, int64_t R, int32_t sample_size, int32_t n_act, float *q, void *stream) {
    if (int rc = iqn_check("tsm_iqn_values", 4, 16, sample_size, n_act)) return rc;
    TSM_REQUIRE(R >= 0 && R <= kIMaxRows, "tsm_iqn_values: R = %lld out of range", (long long)R);
    if (R == 0) return TSM_OK;
    TSM_REQUIRE(out && q, "tsm_iqn_values: null pointer");
    hipLaunchKernelGGL(iqn_values_kernel, dim3((unsigned)ceil_div(R * n_act, kIThreads)), dim3(kIThreads), 0,
                       tsm_stream(stream), out, R, sample_size, n_act, q);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_iqn_head(const float *out, const float *q_next, const float *out_next, const uint8_t *mask_next,
                            const float *taus, const int64_t *act, const float *mc, const float *gpow, const uint8_t *vmask,
                            const float *weight, int64_t B, int32_t n_act, int32_t n_online, int32_t n_target,
                            float *returns_out, float *prio, float *d_out, double *partial, void *stream) {
    if (int rc = iqn_check("tsm_iqn_head", 4, 16, n_online, n_act)) return rc;
    TSM_REQUIRE(n_target >= 2 && n_target <= kIMaxS, "tsm_iqn_head: target sample_size = %d outside [2, %d]", n_target, kIMaxS);
    if (int rc = tsm_q_check_rows("tsm_iqn_head", B)) return rc;
    TSM_REQUIRE(out && q_next && out_next && taus && act && mc && gpow && vmask && returns_out && prio && d_out && partial,
                "tsm_iqn_head: null pointer");
    hipLaunchKernelGGL(iqn_head_kernel, dim3((unsigned)ceil_div(B, TSM_IQN_ROWS_PER_BLOCK)), dim3(kIThreads), 0,
                       tsm_stream(stream), out, q_next, out_next, mask_next, taus, act, mc, gpow, vmask, weight, B, n_act,
                       n_online, n_target, returns_out, prio, d_out, partial);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}
