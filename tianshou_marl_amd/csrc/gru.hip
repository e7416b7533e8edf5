// gru.hip -- the recurrence of a GRU layer, forward and backward through time.
//
// Replaces, for utils/net.Recurrent(cell="gru"):
//   nn.GRU(hidden, hidden, layer_num, batch_first=True) and `loss.backward()` through it: the agent net of the recurrent
//   value-based multi-agent learners (fc -> GRU -> fc), which the reference's `Recurrent` spells with an LSTM.
// torch's layout: gate order r, z, n; weight_hh [3H][H].  The input projection X W_ih^T + b_ih of all B * L rows, the weight
// gradients and d_x = d_gates_x W_ih are row GEMMs and run on csrc/dense.hip (tsm_dense_*); what is here is the part that is
// serial in time:
//   r = sigmoid(x_r + b_hr + h W_hr^T)   z = sigmoid(x_z + b_hz + h W_hz^T)   q = h W_hn^T + b_hn
//   n = tanh(x_n + r q)                  h' = (1 - z) n + z h
//
// Forward: one launch covers all L steps of a layer.  A workgroup owns kGruRows = 16 batch rows (one MFMA M tile) and has
// H / 16 waves; wave w owns the hidden columns [16 w, 16 w + 16) of all three gates, so the r, z and q of one (row, column)
// meet in one lane's accumulators (v_mfma_f32_16x16x4_f32: row (lane >> 4) * 4 + j, column lane & 15) and the update needs no
// exchange.  The reset gate multiplies the recurrent product of the candidate, so q has an accumulator of its own that starts
// from b_hn, and x_n stays beside it in registers until r is known.  The wave's slice of W_hh -- 48 gate rows x H, 3 H / 4
// B-operand registers, 96 at H = 128 -- stays in registers for the whole launch; only h_{t-1} [16][H + 2] goes through LDS
// (two buffers: one barrier per step), and the lane keeps its own h_{t-1} element for the z h term.
//
// Backward: walks t = L-1 .. 0.  With dh = d_h[t] + carried:
//   da_n = dh (1 - z)(1 - n^2)   da_z = dh (h_{t-1} - n) z (1 - z)   da_r = da_n q r (1 - r)
// Two blocks leave the kernel, because the candidate's recurrent product sits behind r and its input projection does not:
//   d_gates_x = {da_r, da_z, da_n}     -> weight_ih, bias_ih, and the layer below
//   d_gates_h = {da_r, da_z, da_n r}   -> weight_hh, bias_hh, and  carried = dh z + d_gates_h W_hh  (K = 3H)
// The wave holds the columns [16 w, 16 w + 16) of W_hh for all 3H rows (3 H / 4 registers) and publishes its d_gates_h columns
// through LDS [16][3H + 2], again in two buffers; the saved rows of step t - 1 are loaded before the product of step t is
// issued, so they fly under it.  No atomics: two runs give the same bits.  f32 products and accumulation throughout.
#include "common.h"

namespace {

constexpr int kGruRows = TSM_GRU_ROWS_PER_BLOCK;

// finite for every finite x without passing through inf: the exponent is never positive, e lies in [0, 1] (as in lstm.hip)
__device__ __forceinline__ float gru_sigmoid(float x) {
    const float e = expf(-fabsf(x));
    return (x >= 0.f ? 1.f : e) / (1.f + e);
}

struct GruFwdArgs {
    const float *proj;   // [B][L][3H]
    const float *w_hh;   // [3H][H]
    const float *bias;   // nullable [3H]: b_hh
    const float *h0;     // nullable, row pitch ld_state
    int64_t ld_state, B;
    int L;
    float *h;                    // [B][L][H]
    float *h_prev, *gates, *q;   // nullable: [B][L][H], [B][L][3H], [B][L][H]
    float *h_n;                  // nullable, row pitch ld_state; may alias h0 (a workgroup reads its rows before it writes them)
};

template <int H>
__global__ __launch_bounds__(H * 4) void gru_forward_kernel(GruFwdArgs a) {
    constexpr int KSTEPS = H / 4, LD = H + 2;
    __shared__ float hs[2][kGruRows * LD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, qd = lane >> 4;
    const int col = wave * 16 + (lane & 15);
    const int64_t row0 = (int64_t)blockIdx.x * kGruRows + qd * 4;   // first of this lane's four rows
    const int64_t G3 = 3 * H;

    float w[3][KSTEPS];   // B operand of gate g, k step s: W_hh[g H + col][4 s + qd]
    float bh[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) {
        const float *wr = a.w_hh + (int64_t)(g * H + col) * H + qd;
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) w[g][s] = wr[4 * s];
        bh[g] = a.bias ? a.bias[g * H + col] : 0.f;
    }

    f4 hst;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t row = row0 + j;
        hst[j] = row < a.B && a.h0 ? a.h0[row * a.ld_state + col] : 0.f;
        hs[0][(qd * 4 + j) * LD + col] = hst[j];
    }
    __syncthreads();

    f4 p[3];   // x_r, x_z, x_n of the step ahead
    auto load_proj = [&](int t, f4 (&dst)[3]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t row = row0 + j;
            const float *pr = a.proj + ((row < a.B ? row : 0) * a.L + t) * G3 + col;
#pragma unroll
            for (int g = 0; g < 3; ++g) {
                const float v = pr[g * H];
                dst[g][j] = row < a.B ? v : 0.f;
            }
        }
    };
    load_proj(0, p);

    int cur = 0;
    for (int t = 0; t < a.L; ++t) {
        f4 acc[3] = {p[0] + bh[0], p[1] + bh[1], f4{bh[2], bh[2], bh[2], bh[2]}};
        const f4 xn = p[2];
        if (t + 1 < a.L) load_proj(t + 1, p);   // the next step's rows fly while this one is multiplied
        const float *at = hs[cur] + (lane & 15) * LD + qd;
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) {
            const float av = at[4 * s];
#pragma unroll
            for (int g = 0; g < 3; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, w[g][s], acc[g], 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t row = row0 + j;
            const float gr = gru_sigmoid(acc[0][j]), gz = gru_sigmoid(acc[1][j]), gq = acc[2][j];
            const float gn = tanhf(xn[j] + gr * gq);
            const float hp = hst[j];
            hst[j] = (1.f - gz) * gn + gz * hp;
            hs[cur ^ 1][(qd * 4 + j) * LD + col] = hst[j];
            if (row < a.B) {
                const int64_t o = (row * a.L + t) * H + col;
                a.h[o] = hst[j];
                if (a.h_prev) a.h_prev[o] = hp;
                if (a.q) a.q[o] = gq;
                if (a.gates) {
                    float *gw = a.gates + (row * a.L + t) * G3 + col;
                    gw[0] = gr; gw[H] = gz; gw[2 * H] = gn;
                }
            }
        }
        __syncthreads();   // h_t is complete before any wave multiplies it; the other buffer was last read a step ago
        cur ^= 1;
    }
    if (a.h_n) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t row = row0 + j;
            if (row < a.B) a.h_n[row * a.ld_state + col] = hst[j];
        }
    }
}

struct GruBwdArgs {
    const float *d_h;    // [B][L][H]
    const float *d_hn;   // nullable, row pitch ld_state
    const float *w_hh;   // [3H][H]
    const float *gates, *q, *h_prev;   // saved by the forward
    int64_t ld_state, B;
    int L;
    float *d_gates_x, *d_gates_h;   // [B][L][3H] each
    float *d_h0;                    // nullable, row pitch ld_state
};

struct GruSaved {   // what one step of the backward reads, for this lane's four rows
    f4 r, z, n, q, hp, dh;
};

template <int H>
__global__ __launch_bounds__(H * 4) void gru_backward_kernel(GruBwdArgs a) {
    constexpr int KSTEPS = 3 * H / 4, LD = 3 * H + 2;   // K = 3H
    __shared__ float dgs[2][kGruRows * LD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, qd = lane >> 4;
    const int col = wave * 16 + (lane & 15);
    const int64_t row0 = (int64_t)blockIdx.x * kGruRows + qd * 4;
    const int64_t G3 = 3 * H;

    float w[KSTEPS];   // B operand of k step s: W_hh[4 s + qd][col]
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) w[s] = a.w_hh[(int64_t)(4 * s + qd) * H + col];

    f4 carried;   // d loss / d h_t from step t + 1: dh z + d_gates_h W_hh
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t row = row0 + j;
        carried[j] = row < a.B && a.d_hn ? a.d_hn[row * a.ld_state + col] : 0.f;
    }

    auto load_step = [&](int t, GruSaved &s) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t row = row0 + j;
            const bool ok = row < a.B;
            const int64_t o = ((ok ? row : 0) * a.L + t) * H + col;
            const float *gr = a.gates + ((ok ? row : 0) * a.L + t) * G3 + col;
            const float r = gr[0], z = gr[H], n = gr[2 * H], qv = a.q[o], hp = a.h_prev[o], dh = a.d_h[o];
            s.r[j] = ok ? r : 0.f; s.z[j] = ok ? z : 0.f; s.n[j] = ok ? n : 0.f;
            s.q[j] = ok ? qv : 0.f; s.hp[j] = ok ? hp : 0.f; s.dh[j] = ok ? dh : 0.f;
        }
    };
    GruSaved sv;
    load_step(a.L - 1, sv);

    int cur = 0;
    for (int t = a.L - 1; t >= 0; --t) {
        const GruSaved s = sv;
        if (t > 0) load_step(t - 1, sv);   // the saved rows of the step before fly under this step's product
        f4 dhz;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t row = row0 + j;
            const float dh = s.dh[j] + carried[j];   // a row past B: zeros in, zeros out
            const float dn = dh * (1.f - s.z[j]) * (1.f - s.n[j] * s.n[j]);
            const float dz = dh * (s.hp[j] - s.n[j]) * (s.z[j] * (1.f - s.z[j]));
            const float dr = dn * s.q[j] * (s.r[j] * (1.f - s.r[j]));
            const float dnr = dn * s.r[j];
            dhz[j] = dh * s.z[j];
            float *ls = dgs[cur] + (qd * 4 + j) * LD + col;
            ls[0] = dr; ls[H] = dz; ls[2 * H] = dnr;
            if (row < a.B) {
                const int64_t o = (row * a.L + t) * G3 + col;
                float *gx = a.d_gates_x + o, *gh = a.d_gates_h + o;
                gx[0] = dr; gx[H] = dz; gx[2 * H] = dn;
                gh[0] = dr; gh[H] = dz; gh[2 * H] = dnr;
            }
        }
        __syncthreads();   // d_gates_h of step t is complete; the other buffer was last read a step ago
        // four accumulators walk the k range a quarter each: the dependent-accumulator latency of the MFMA stays hidden
        f4 acc[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] = f4{0.f, 0.f, 0.f, 0.f};
        const float *at = dgs[cur] + (lane & 15) * LD + qd;
#pragma unroll
        for (int k = 0; k < KSTEPS; ++k) acc[k & 3] = __builtin_amdgcn_mfma_f32_16x16x4f32(at[4 * k], w[k], acc[k & 3], 0, 0, 0);
        carried = dhz + ((acc[0] + acc[1]) + (acc[2] + acc[3]));
        cur ^= 1;
    }
    if (a.d_h0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t row = row0 + j;
            if (row < a.B) a.d_h0[row * a.ld_state + col] = carried[j];
        }
    }
}

template <int H>
void launch_fwd(const GruFwdArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(gru_forward_kernel<H>, dim3((unsigned)ceil_div(a.B, kGruRows)), dim3(H * 4), 0, s, a);
}
template <int H>
void launch_bwd(const GruBwdArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(gru_backward_kernel<H>, dim3((unsigned)ceil_div(a.B, kGruRows)), dim3(H * 4), 0, s, a);
}

int gru_dims(const char *who, int64_t B, int32_t L, int32_t H) {
    if (int rc = tsm_gru_check(H, 1, L)) return rc;
    TSM_REQUIRE(B >= 1 && ceil_div(B, kGruRows) <= 2147483647LL, "%s: batch %lld out of range", who, (long long)B);
    TSM_REQUIRE((int64_t)B * L <= (int64_t)1 << 40, "%s: B * L = %lld rows too many", who, (long long)B * L);
    return TSM_OK;
}

}  // namespace

TSM_EXPORT int tsm_gru_check(int32_t hidden, int32_t layer_num, int32_t seq_len) {
    TSM_REQUIRE(hidden >= 16 && hidden <= TSM_GRU_MAX_HIDDEN && hidden % 16 == 0,
                "gru: hidden size %d must be a multiple of 16 in [16, %d]", hidden, TSM_GRU_MAX_HIDDEN);
    TSM_REQUIRE(layer_num >= 1, "gru: layer_num %d must be >= 1", layer_num);
    TSM_REQUIRE(seq_len >= 1, "gru: sequence length %d must be >= 1", seq_len);
    return TSM_OK;
}

#define TSM_GRU_DISPATCH(fn, H, ...)                    \
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
        tsm_set_error("gru: no kernel for hidden size %d", (int)(H)); \
        return TSM_ERR_INVALID;                         \
    }

TSM_EXPORT int tsm_gru_forward(const float *proj, const float *w_hh, const float *bias, const float *h0, int64_t ld_state,
                               int64_t B, int32_t L, int32_t H, float *h, float *h_prev, float *gates, float *q, float *h_n,
                               void *stream) {
    if (int rc = gru_dims("tsm_gru_forward", B, L, H)) return rc;
    TSM_REQUIRE(proj && w_hh && h, "tsm_gru_forward: null pointer");
    TSM_REQUIRE(!(h0 || h_n) || ld_state >= H, "tsm_gru_forward: ld_state %lld smaller than H = %d", (long long)ld_state, H);
    GruFwdArgs a{proj, w_hh, bias, h0, ld_state, B, L, h, h_prev, gates, q, h_n};
    TSM_GRU_DISPATCH(launch_fwd, H, a, tsm_stream(stream));
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_gru_backward(const float *d_h, const float *d_hn, const float *w_hh, const float *gates, const float *q,
                                const float *h_prev, int64_t ld_state, int64_t B, int32_t L, int32_t H, float *d_gates_x,
                                float *d_gates_h, float *d_h0, void *stream) {
    if (int rc = gru_dims("tsm_gru_backward", B, L, H)) return rc;
    TSM_REQUIRE(d_h && w_hh && gates && q && h_prev && d_gates_x && d_gates_h, "tsm_gru_backward: null pointer");
    TSM_REQUIRE(!(d_hn || d_h0) || ld_state >= H, "tsm_gru_backward: ld_state %lld smaller than H = %d", (long long)ld_state, H);
    GruBwdArgs a{d_h, d_hn, w_hh, gates, q, h_prev, ld_state, B, L, d_gates_x, d_gates_h, d_h0};
    TSM_GRU_DISPATCH(launch_bwd, H, a, tsm_stream(stream));
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}
