// lstm.hip -- the recurrence of an LSTM layer, forward and backward through time, and the state reset of finished envs.
//
// Replaces, for utils/net.Recurrent:
//   nn.LSTM(hidden, hidden, layer_num, batch_first=True)      /root/reference/tianshou/utils/net/common.py:389-394, 433-446
//   and `loss.backward()` through it.
// torch's layout: gate order i, f, g, o; weight_hh [4H][H].  The input projection X W_ih^T + b_ih of all B * L rows, the
// weight gradients and d_x = d_gates W_ih are row GEMMs and run on csrc/dense.hip (tsm_dense_*); what is here is the part
// that is serial in time.
//
// One launch covers all L steps of a layer.  Batch rows are independent: a workgroup owns kLstmRows = 16 rows (one MFMA
// M tile) and carries their h and c through time.  It has H / 16 waves; wave w owns the hidden columns [16 w, 16 w + 16)
// of all four gates, so the i, f, g, o of one (row, column) meet in one lane's accumulators (v_mfma_f32_16x16x4_f32: row
// (lane >> 4) * 4 + r, column lane & 15) and the cell update needs no exchange.  The wave's slice of W_hh -- 64 gate rows x H,
// H / 4 B-operand registers per gate, 128 registers at H = 128 -- stays in registers for the whole launch; only h_{t-1}
// [16][H] goes through LDS, as the A operand every wave reads (row stride H + 2 words = 2 x odd: conflict-free for the
// operand pattern lane -> [lane & 15][lane >> 4], as in dense.hip).  f32 products and accumulation throughout.
//
// The backward walks t = L-1 .. 0 with the transposed product d_h_{t-1} += d_gates_t W_hh (K = 4H): the wave holds the
// columns [16 w, 16 w + 16) of W_hh for all 4H gate rows (H registers), forms the d_gates of its own columns elementwise
// from the saved activated gates and cell states, and publishes them through LDS [16][4H + 2] as the A operand.
#include "common.h"

namespace {

constexpr int kLstmRows = TSM_LSTM_ROWS_PER_BLOCK;

// finite for every finite x without passing through inf: the exponent is never positive, e lies in [0, 1]
__device__ __forceinline__ float lstm_sigmoid(float x) {
    const float e = expf(-fabsf(x));
    return (x >= 0.f ? 1.f : e) / (1.f + e);
}

struct LstmFwdArgs {
    const float *proj;   // [B][L][4H]
    const float *w_hh;   // [4H][H]
    const float *bias;   // nullable [4H], added to proj
    const float *h0, *c0;  // nullable, row pitch ld_state
    int64_t ld_state, B;
    int L;
    float *h;            // [B][L][H]
    float *h_prev, *gates, *c;  // nullable: [B][L][H], [B][L][4H], [B][L][H]
    float *h_n, *c_n;    // nullable, row pitch ld_state; may alias h0 / c0 (a workgroup reads its rows before it writes them)
};

template <int H>
__global__ __launch_bounds__(H * 4) void lstm_forward_kernel(LstmFwdArgs a) {
    constexpr int KSTEPS = H / 4, LD = H + 2;
    __shared__ float hs[2][kLstmRows * LD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4;
    const int col = wave * 16 + (lane & 15);
    const int64_t row0 = (int64_t)blockIdx.x * kLstmRows + q * 4;   // first of this lane's four rows

    float w[4][KSTEPS];   // B operand of gate g, k step s: W_hh[g H + col][4 s + q]
    float bsum[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float *wr = a.w_hh + (int64_t)(g * H + col) * H + q;
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) w[g][s] = wr[4 * s];
        bsum[g] = a.bias ? a.bias[g * H + col] : 0.f;
    }

    f4 cst, hst;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t row = row0 + j;
        const bool ok = row < a.B;
        cst[j] = ok && a.c0 ? a.c0[row * a.ld_state + col] : 0.f;
        hst[j] = ok && a.h0 ? a.h0[row * a.ld_state + col] : 0.f;
        hs[0][(q * 4 + j) * LD + col] = hst[j];
    }
    __syncthreads();

    const int64_t G4 = 4 * H;
    f4 p[4];
    auto load_proj = [&](int t, f4 (&dst)[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t row = row0 + j;
            const float *pr = a.proj + ((row < a.B ? row : 0) * a.L + t) * G4 + col;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float v = pr[g * H];
                dst[g][j] = row < a.B ? v + bsum[g] : 0.f;
            }
        }
    };
    load_proj(0, p);

    int cur = 0;
    for (int t = 0; t < a.L; ++t) {
        f4 acc[4] = {p[0], p[1], p[2], p[3]};
        if (t + 1 < a.L) load_proj(t + 1, p);   // the next step's rows fly while this one is multiplied
        const float *at = hs[cur] + (lane & 15) * LD + q;
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) {
            const float av = at[4 * s];
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, w[g][s], acc[g], 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t row = row0 + j;
            const float gi = lstm_sigmoid(acc[0][j]), gf = lstm_sigmoid(acc[1][j]);
            const float gg = tanhf(acc[2][j]), go = lstm_sigmoid(acc[3][j]);
            const float hp = hst[j];
            cst[j] = gf * cst[j] + gi * gg;
            hst[j] = go * tanhf(cst[j]);
            hs[cur ^ 1][(q * 4 + j) * LD + col] = hst[j];
            if (row < a.B) {
                const int64_t o = (row * a.L + t) * H + col;
                a.h[o] = hst[j];
                if (a.h_prev) a.h_prev[o] = hp;
                if (a.c) a.c[o] = cst[j];
                if (a.gates) {
                    float *gr = a.gates + (row * a.L + t) * G4 + col;
                    gr[0] = gi; gr[H] = gf; gr[2 * H] = gg; gr[3 * H] = go;
                }
            }
        }
        __syncthreads();   // h_t is complete before any wave multiplies it; the other buffer was last read a step ago
        cur ^= 1;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t row = row0 + j;
        if (row >= a.B) continue;
        if (a.h_n) a.h_n[row * a.ld_state + col] = hst[j];
        if (a.c_n) a.c_n[row * a.ld_state + col] = cst[j];
    }
}

struct LstmBwdArgs {
    const float *d_h;          // [B][L][H]
    const float *d_hn, *d_cn;  // nullable, row pitch ld_state
    const float *w_hh;         // [4H][H]
    const float *gates, *c;    // saved by the forward
    const float *c0;           // nullable, row pitch ld_state
    int64_t ld_state, B;
    int L;
    float *d_gates;            // [B][L][4H]
    float *d_h0, *d_c0;        // nullable, row pitch ld_state
};

template <int H>
__global__ __launch_bounds__(H * 4) void lstm_backward_kernel(LstmBwdArgs a) {
    constexpr int KSTEPS = H, LD = 4 * H + 2;   // K = 4H
    __shared__ float dgs[kLstmRows * LD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4;
    const int col = wave * 16 + (lane & 15);
    const int64_t row0 = (int64_t)blockIdx.x * kLstmRows + q * 4;
    const int64_t G4 = 4 * H;

    float w[KSTEPS];   // B operand of k step s: W_hh[4 s + q][col]
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) w[s] = a.w_hh[(int64_t)(4 * s + q) * H + col];

    f4 dc, dhr;   // d loss / d c_t carried from step t + 1, and d_gates_{t+1} W_hh
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t row = row0 + j;
        const bool ok = row < a.B;
        dc[j] = ok && a.d_cn ? a.d_cn[row * a.ld_state + col] : 0.f;
        dhr[j] = ok && a.d_hn ? a.d_hn[row * a.ld_state + col] : 0.f;
    }

    for (int t = a.L - 1; t >= 0; --t) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t row = row0 + j;
            const bool ok = row < a.B;
            const int64_t r = ok ? row : 0;
            const int64_t o = (r * a.L + t) * H + col;
            const float *gr = a.gates + (r * a.L + t) * G4 + col;
            const float gi = gr[0], gf = gr[H], gg = gr[2 * H], go = gr[3 * H];
            const float ct = a.c[o];
            const float cp = t > 0 ? a.c[o - H] : (a.c0 ? a.c0[r * a.ld_state + col] : 0.f);
            const float dh = ok ? a.d_h[o] + dhr[j] : 0.f;
            const float tc = tanhf(ct);
            const float dct = dc[j] + dh * go * (1.f - tc * tc);
            const float di = dct * gg * (gi * (1.f - gi));
            const float df = dct * cp * (gf * (1.f - gf));
            const float dg = dct * gi * (1.f - gg * gg);
            const float dout = dh * tc * (go * (1.f - go));
            dc[j] = ok ? dct * gf : 0.f;
            float *ls = dgs + (q * 4 + j) * LD + col;
            ls[0] = ok ? di : 0.f; ls[H] = ok ? df : 0.f; ls[2 * H] = ok ? dg : 0.f; ls[3 * H] = ok ? dout : 0.f;
            if (ok) {
                float *gw = a.d_gates + (row * a.L + t) * G4 + col;
                gw[0] = di; gw[H] = df; gw[2 * H] = dg; gw[3 * H] = dout;
            }
        }
        __syncthreads();
        // four accumulators walk the k range a quarter each: the dependent-accumulator latency of the MFMA stays hidden
        f4 acc[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] = f4{0.f, 0.f, 0.f, 0.f};
        const float *at = dgs + (lane & 15) * LD + q;
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) acc[s & 3] = __builtin_amdgcn_mfma_f32_16x16x4f32(at[4 * s], w[s], acc[s & 3], 0, 0, 0);
        dhr = (acc[0] + acc[1]) + (acc[2] + acc[3]);
        __syncthreads();   // every wave has read d_gates_t before the next step overwrites it
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t row = row0 + j;
        if (row >= a.B) continue;
        if (a.d_h0) a.d_h0[row * a.ld_state + col] = dhr[j];
        if (a.d_c0) a.d_c0[row * a.ld_state + col] = dc[j];
    }
}

__global__ void lstm_state_reset_kernel(float *h, float *c, const uint8_t *__restrict__ done, int64_t E, int64_t per_env) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= E * per_env) return;
    if (done[i / per_env]) {
        h[i] = 0.f;
        c[i] = 0.f;
    }
}

template <int H>
void launch_fwd(const LstmFwdArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(lstm_forward_kernel<H>, dim3((unsigned)ceil_div(a.B, kLstmRows)), dim3(H * 4), 0, s, a);
}
template <int H>
void launch_bwd(const LstmBwdArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(lstm_backward_kernel<H>, dim3((unsigned)ceil_div(a.B, kLstmRows)), dim3(H * 4), 0, s, a);
}

int lstm_dims(const char *who, int64_t B, int32_t L, int32_t H) {
    if (int rc = tsm_lstm_check(H, 1, L)) return rc;
    TSM_REQUIRE(B >= 1 && ceil_div(B, kLstmRows) <= 2147483647LL, "%s: batch %lld out of range", who, (long long)B);
    TSM_REQUIRE((int64_t)B * L <= (int64_t)1 << 40, "%s: B * L = %lld rows too many", who, (long long)B * L);
    return TSM_OK;
}

}  // namespace

TSM_EXPORT int tsm_lstm_check(int32_t hidden, int32_t layer_num, int32_t seq_len) {
    TSM_REQUIRE(hidden >= 16 && hidden <= TSM_LSTM_MAX_HIDDEN && hidden % 16 == 0,
                "lstm: hidden size %d must be a multiple of 16 in [16, %d]", hidden, TSM_LSTM_MAX_HIDDEN);
    TSM_REQUIRE(layer_num >= 1, "lstm: layer_num %d must be >= 1", layer_num);
    TSM_REQUIRE(seq_len >= 1, "lstm: sequence length %d must be >= 1", seq_len);
    return TSM_OK;
}

#define TSM_LSTM_DISPATCH(fn, H, ...)                   \
    switch (H) {                                        \
    case 16: fn<16>(__VA_ARGS__); break;                \
    case 32: fn<32>(__VA_ARGS__); break;                \
    case 48: fn<48>(__VA_ARGS__); break;                \
    case 64: fn<64>(__VA_ARGS__); break;                \
    case 80: fn<80>(__VA_ARGS__); break;                \
    case 96: fn<96>(__VA_ARGS__); break;                \
    case 112: fn<112>(__VA_ARGS__); break;              \
    case 128: fn<128>(__VA_ARGS__); break;              \
    default:                                            \
        tsm_set_error("lstm: no kernel for hidden size %d", (int)(H)); \
        return TSM_ERR_INVALID;                         \
    }

TSM_EXPORT int tsm_lstm_forward(const float *proj, const float *w_hh, const float *bias, const float *h0, const float *c0,
                                int64_t ld_state, int64_t B, int32_t L, int32_t H, float *h, float *h_prev, float *gates,
                                float *c, float *h_n, float *c_n, void *stream) {
    if (int rc = lstm_dims("tsm_lstm_forward", B, L, H)) return rc;
    TSM_REQUIRE(proj && w_hh && h, "tsm_lstm_forward: null pointer");
    TSM_REQUIRE(!(h0 || c0 || h_n || c_n) || ld_state >= H, "tsm_lstm_forward: ld_state %lld smaller than H = %d",
                (long long)ld_state, H);
    LstmFwdArgs a{proj, w_hh, bias, h0, c0, ld_state, B, L, h, h_prev, gates, c, h_n, c_n};
    TSM_LSTM_DISPATCH(launch_fwd, H, a, tsm_stream(stream));
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_lstm_backward(const float *d_h, const float *d_hn, const float *d_cn, const float *w_hh, const float *gates,
                                 const float *c, const float *c0, int64_t ld_state, int64_t B, int32_t L, int32_t H,
                                 float *d_gates, float *d_h0, float *d_c0, void *stream) {
    if (int rc = lstm_dims("tsm_lstm_backward", B, L, H)) return rc;
    TSM_REQUIRE(d_h && w_hh && gates && c && d_gates, "tsm_lstm_backward: null pointer");
    TSM_REQUIRE(!(d_hn || d_cn || c0 || d_h0 || d_c0) || ld_state >= H, "tsm_lstm_backward: ld_state %lld smaller than H = %d",
                (long long)ld_state, H);
    LstmBwdArgs a{d_h, d_hn, d_cn, w_hh, gates, c, c0, ld_state, B, L, d_gates, d_h0, d_c0};
    TSM_LSTM_DISPATCH(launch_bwd, H, a, tsm_stream(stream));
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_lstm_state_reset(float *h, float *c, const uint8_t *done, int64_t n_env, int64_t rows_per_env,
                                    int64_t row_elems, void *stream) {
    TSM_REQUIRE(n_env >= 0 && rows_per_env >= 1 && row_elems >= 1, "tsm_lstm_state_reset: bad sizes");
    if (n_env == 0) return TSM_OK;
    TSM_REQUIRE(h && c && done, "tsm_lstm_state_reset: null pointer");
    const int64_t per_env = rows_per_env * row_elems, n = n_env * per_env;
    TSM_REQUIRE(ceil_div(n, 256) <= 2147483647LL, "tsm_lstm_state_reset: state too large for one launch");
    hipLaunchKernelGGL(lstm_state_reset_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, tsm_stream(stream), h, c, done,
                       n_env, per_env);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}
