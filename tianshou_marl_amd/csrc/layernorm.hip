// layernorm.hip -- fully-connected networks whose hidden layers are Linear -> LayerNorm -> activation.
//
// Replaces  MLP(norm_layer=nn.LayerNorm) of the reference (tianshou/utils/net/common.py:22-47, 90-169: the norm layer sits
//           between every hidden Linear and its activation; the last layer is a plain Linear) and `loss.backward()` through it.
// Parameter vector = torch `parameters()` order: hidden layer l  w_l [O][K], b_l [O], gamma_l [O], beta_l [O]; last layer w, b.
//
// Per hidden layer and row (O = the layer's width):
//   y = x W^T + b;  mu = mean_j y;  var = mean_j (y - mu)^2 (biased, two-pass on the values in registers);
//   rstd = 1 / sqrt(var + eps);  xhat = (y - mu) rstd;  p = gamma xhat + beta;  a = act(p)
//
// ln_fwd_kernel: GEMM + bias + LayerNorm + affine + activation in ONE launch per normalised layer.
//   A workgroup of 4 waves owns 16 rows and ALL O columns.  The ceil(O / 16) column tiles of 16 are dealt to the waves in
//   contiguous runs of TPW = 1, 2, 4 or 8 tiles (the smallest run with 4 TPW >= the tile count; wave w owns tiles
//   [w TPW, (w + 1) TPW), those behind the last column multiply zeros).  v_mfma_f32_16x16x4_f32, as dense.hip: exact f32 products.
//   The k loop stages the 16 x 16 piece of x and the (64 TPW) x 16 piece of W through LDS with gemm_tile_dev.h's row-major
//   loader (row stride 18 words; one unconditional 16-byte load per thread where the piece is inside and aligned, guarded
//   loads at the edges: no alignment is asked of the caller), double buffered.
//   Epilogue, in a fixed order: bias; a row's sum first across the 16 lanes that hold its columns of one C fragment
//   (register r of lane l holds C[(l >> 4) * 4 + r][l & 15]; DPP row rotations 8, 4, 2, 1), then across the wave's tiles in
//   tile order, then across the four waves through LDS in wave order.  The same order serves the mean and, on y - mu, the
//   variance.  A row's bits depend on neither B nor the other rows.
//   Writes a into the `acts` block (the next layer's input) and, where `saved` is given, xhat [B][O] and rstd [B]: the backward
//   needs exactly these two (p is gamma xhat + beta again, dy is a function of xhat and rstd); keeping y, mu, rstd instead would
//   cost the backward the subtraction and product per element and one more float per row.
//   Width cap TSM_LN_MAX_WIDTH = 512: the accumulators are O / 16 = 32 VGPRs per lane, the prefetch registers of the W piece 32
//   more, and the two W tiles of the double buffer are 2 x 512 x 18 words = 73.7 KB of the 160 KB of LDS (two workgroups per CU).
//   Wider layers are refused; there is no second, two-launch forward path.
//
// ln_bwd_rows_kernel: da, xhat, rstd, gamma, beta -> dy [B][O] (in place over da) and the gamma / beta gradients of the slabs.
//   dp = da act'(p), p recomputed by the forward's f32 expression (so a ReLU mask agrees bit for bit);
//   dgamma = sum_b dp xhat;  dbeta = sum_b dp;  dxhat = dp gamma;
//   dy = rstd (dxhat - mean_j dxhat - xhat mean_j (dxhat xhat))
//   ONE workgroup of 16 waves per slab (slab ranges are dense's: k_per = ceil(ceil(B / n_split) / 16) * 16 rows), so a slab's
//   columns have one writer and no second launch folds workgroup partials.  Wave w walks rows r0 + w, r0 + w + 16, ... one at a
//   time; lane l holds columns l, l + 64, ... (at most 8 at 512) in registers; the two row means are a per-lane sum over its
//   columns in order, then the xor butterfly 32, 16, 8, 4, 2, 1.  Each lane accumulates dp xhat and dp of its columns over the
//   rows it walked; the waves fold through LDS in wave order.  Every slab's gamma / beta entries are written on every call
//   (a slab without rows: +0.0).  with_params = 0 leaves the parameter gradients out (the input-gradient chain); the grid is
//   then one workgroup per 16 rows.  No atomics anywhere: results are bit-reproducible.
//
// Host chains: tsm_mlp_ln_forward / _backward / _input_grad.  The plain GEMMs of the chains (last layer's forward, da = dz W,
// weight and bias gradients from dy) are dense.hip's instantiations, launched through tsm_dense_*.
#include "common.h"
#include "gemm_tile_dev.h"

namespace {

constexpr int LN_ROWS = 16;        // rows of a forward workgroup: one MFMA tile
constexpr int LN_BWD_WAVES = 16;   // waves of a backward workgroup
constexpr int LN_MAX_J = TSM_LN_MAX_WIDTH / kWave;  // columns a lane of the row kernel holds
static_assert(BK == 16 && NT == 256, "the forward reuses the 64 x 16 row-major loader of gemm_tile_dev.h");

struct LnFwdArgs {
    const float *X;                       // [M][K]
    const float *W, *bias, *gamma, *beta; // [O][K], [O], [O], [O]
    int64_t M;
    int32_t K, O, act;
    float eps;
    float *out;                           // [M][O]
    float *xhat, *rstd;                   // nullable together: [M][O], [M]
};

template <int TPW>
__global__ __launch_bounds__(NT) void ln_fwd_kernel(LnFwdArgs g) {
    constexpr int WR = 64 * TPW;               // rows of W staged per k tile: >= O, zeros behind it
    constexpr int kTile = (LN_ROWS + WR) * LDT;  // one x tile + one W tile
    extern __shared__ __attribute__((aligned(16))) float ln_lds[];
    __shared__ float red[2][4][LN_ROWS];       // per wave row sums: [0] of y, [1] of (y - mu)^2
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t m0 = (int64_t)blockIdx.x * LN_ROWS;
    const int64_t K = g.K, O = g.O;
    const int64_t n_iter = (K + BK - 1) / BK;

    f4 acc[TPW];
#pragma unroll
    for (int t = 0; t < TPW; ++t) acc[t] = f4{0.f, 0.f, 0.f, 0.f};

    const auto al16 = [](const float *p, int64_t ld) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && (ld & 3) == 0; };
    const bool x_in = al16(g.X, K) && m0 + LN_ROWS <= g.M;
    const bool w_al = al16(g.W, K);
    float va[4], vb[TPW][4];
    auto fetch = [&](int64_t k0) {
        const bool k_in = k0 + BK <= K;
        if (tid < 4 * LN_ROWS) load_rowmajor(g.X, K, m0, g.M, k0, K, va, tid, x_in && k_in);   // wave 0: rows tid >> 2
#pragma unroll
        for (int p = 0; p < TPW; ++p)
            load_rowmajor(g.W, K, 64 * p, O, k0, K, vb[p], tid, w_al && k_in && 64 * (p + 1) <= O);
    };
    auto commit = [&](int buf) {
        float *xt = ln_lds + buf * kTile, *wt = xt + LN_ROWS * LDT;
        if (tid < 4 * LN_ROWS) store_rowmajor(xt, va, tid, 0);
#pragma unroll
        for (int p = 0; p < TPW; ++p) store_rowmajor(wt + 64 * p * LDT, vb[p], tid, 0);
    };

    int buf = 0;
    fetch(0);
    commit(0);
    __syncthreads();
    for (int64_t it = 0; it < n_iter; ++it) {
        const bool more = it + 1 < n_iter;
        if (more) fetch((it + 1) * BK);  // global loads of the next tile fly while this one is multiplied
        const float *a_t = ln_lds + buf * kTile + (lane & 15) * LDT + (lane >> 4);
        const float *b_t = ln_lds + buf * kTile + LN_ROWS * LDT + (wave * TPW * 16 + (lane & 15)) * LDT + (lane >> 4);
#pragma unroll
        for (int kk = 0; kk < BK; kk += 4) {
            const float a = a_t[kk];
#pragma unroll
            for (int t = 0; t < TPW; ++t)
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b_t[t * 16 * LDT + kk], acc[t], 0, 0, 0);
        }
        if (more) commit(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }

    // C fragment: register r of lane l holds C[(l >> 4) * 4 + r][l & 15]
    const int cl = lane & 15, rq = lane >> 4;
    bool c_ok[TPW];
    float ga[TPW], be[TPW];
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        const int col = (wave * TPW + t) * 16 + cl;
        c_ok[t] = col < g.O;
        const float b = c_ok[t] ? g.bias[col] : 0.f;
        ga[t] = c_ok[t] ? g.gamma[col] : 0.f;
        be[t] = c_ok[t] ? g.beta[col] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[t][r] = c_ok[t] ? acc[t][r] + b : 0.f;
    }
    const float n_col = (float)g.O;
    float mu[4], rs[4];
    {   // mean: lanes of a fragment row, then the wave's tiles, then the waves
        float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < TPW; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) s[r] += row16_sum(acc[t][r]);
        if (cl == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) red[0][wave][rq * 4 + r] = s[r];
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = rq * 4 + r;
            mu[r] = (((red[0][0][i] + red[0][1][i]) + red[0][2][i]) + red[0][3][i]) / n_col;
        }
    }
    {   // biased variance of the values in registers, same order
        float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < TPW; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float d = c_ok[t] ? acc[t][r] - mu[r] : 0.f;
                acc[t][r] = d;
                s[r] += row16_sum(d * d);
            }
        if (cl == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) red[1][wave][rq * 4 + r] = s[r];
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = rq * 4 + r;
            const float var = (((red[1][0][i] + red[1][1][i]) + red[1][2][i]) + red[1][3][i]) / n_col;
            rs[r] = 1.f / sqrtf(var + g.eps);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t row = m0 + rq * 4 + r;
        if (row >= g.M) continue;
        if (g.rstd && wave == 0 && cl == 0) g.rstd[row] = rs[r];
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
            if (!c_ok[t]) continue;
            const int64_t e = row * O + (wave * TPW + t) * 16 + cl;
            const float xh = acc[t][r] * rs[r];
            if (g.xhat) g.xhat[e] = xh;
            g.out[e] = act_fwd(ga[t] * xh + be[t], g.act);
        }
    }
}

struct LnBwdArgs {
    const float *da;                 // [B][O]
    float *dy;                       // [B][O]; may be da itself (an element is read and written by the same lane)
    const float *xhat, *rstd, *gamma, *beta;
    int64_t B, k_per;                // rows of one workgroup: [blockIdx.x * k_per, +k_per) cut at B
    int32_t O, act, with_params;
    float *slabs;                    // with_params: slab blockIdx.x receives dgamma at g_off, dbeta at be_off
    int64_t slab_stride, g_off, be_off;
};

__global__ __launch_bounds__(LN_BWD_WAVES * kWave) void ln_bwd_rows_kernel(LnBwdArgs g) {
    __shared__ float fold[2][TSM_LN_MAX_WIDTH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t O = g.O;
    const int64_t r0 = (int64_t)blockIdx.x * g.k_per;
    const int64_t r1 = r0 + g.k_per < g.B ? r0 + g.k_per : g.B;
    const float n_col = (float)g.O;
    float ga[LN_MAX_J], be[LN_MAX_J], g_acc[LN_MAX_J], b_acc[LN_MAX_J];
#pragma unroll
    for (int j = 0; j < LN_MAX_J; ++j) {
        const int c = lane + kWave * j;
        ga[j] = c < g.O ? g.gamma[c] : 0.f;
        be[j] = c < g.O ? g.beta[c] : 0.f;
        g_acc[j] = b_acc[j] = 0.f;
    }
    float xh[LN_MAX_J], dd[LN_MAX_J];
    auto fetch = [&](int64_t row) {
#pragma unroll
        for (int j = 0; j < LN_MAX_J; ++j) {
            const int c = lane + kWave * j;
            const bool ok = c < g.O && row < r1;
            xh[j] = ok ? g.xhat[row * O + c] : 0.f;
            dd[j] = ok ? g.da[row * O + c] : 0.f;
        }
    };
    fetch(r0 + wave);
    for (int64_t row = r0 + wave; row < r1; row += LN_BWD_WAVES) {
        float x[LN_MAX_J], dxh[LN_MAX_J];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int j = 0; j < LN_MAX_J; ++j) {   // (a column behind the width holds zeros throughout: it adds +0.0)
            x[j] = xh[j];
            const float a = act_fwd(ga[j] * x[j] + be[j], g.act);
            const float dp = dd[j] * act_bwd(a, g.act);
            g_acc[j] += dp * x[j];
            b_acc[j] += dp;
            dxh[j] = dp * ga[j];
            s1 += dxh[j];
            s2 += dxh[j] * x[j];
        }
        const float rs = g.rstd[row];
        fetch(row + LN_BWD_WAVES);             // the next row's loads fly over the butterfly and the stores
        const float m1 = wave_sum(s1) / n_col, m2 = wave_sum(s2) / n_col;
#pragma unroll
        for (int j = 0; j < LN_MAX_J; ++j) {
            const int c = lane + kWave * j;
            if (c < g.O) g.dy[row * O + c] = rs * ((dxh[j] - m1) - x[j] * m2);
        }
    }
    if (!g.with_params) return;   // workgroup-uniform
    for (int w = 0; w < LN_BWD_WAVES; ++w) {   // the waves fold in wave order
        if (wave == w) {
#pragma unroll
            for (int j = 0; j < LN_MAX_J; ++j) {
                const int c = lane + kWave * j;
                if (c < g.O) {
                    fold[0][c] = w == 0 ? g_acc[j] : fold[0][c] + g_acc[j];
                    fold[1][c] = w == 0 ? b_acc[j] : fold[1][c] + b_acc[j];
                }
            }
        }
        __syncthreads();
    }
    float *dst = g.slabs + (int64_t)blockIdx.x * g.slab_stride;
    for (int c = tid; c < g.O; c += LN_BWD_WAVES * kWave) {
        dst[g.g_off + c] = fold[0][c];
        dst[g.be_off + c] = fold[1][c];
    }
}

int ln_check(const tsm_mlp_desc *d, const char *who) {
    if (int rc = check_desc(d, who)) return rc;
    for (int l = 1; l < d->n_layers; ++l)
        TSM_REQUIRE(d->dims[l] <= TSM_LN_MAX_WIDTH, "%s: normalised layer %d is %d wide; the one-launch LayerNorm forward holds a whole "
                    "row in one workgroup and serves widths up to %d", who, l, d->dims[l], TSM_LN_MAX_WIDTH);
    return TSM_OK;
}

// offsets of each layer's W (b behind it, then gamma, beta of a hidden layer), of the block of `acts` holding its output and
// of its xhat block in `saved` (rstd behind it); -> parameter count
int64_t ln_offsets(const tsm_mlp_desc *d, int64_t B, int64_t *p_off, int64_t *a_off, int64_t *s_off) {
    int64_t po = 0, ao = 0, so = 0;
    for (int l = 0; l < d->n_layers; ++l) {
        const int64_t K = d->dims[l], O = d->dims[l + 1];
        p_off[l] = po;
        a_off[l] = ao;
        s_off[l] = so;
        po += O * K + O;
        ao += B * O;
        if (l + 1 < d->n_layers) {
            po += 2 * O;
            so += B * O + B;
        }
    }
    return po;
}

template <int TPW>
int ln_fwd_launch(const LnFwdArgs &g, hipStream_t stream) {
    constexpr size_t lds = 2 * (size_t)(LN_ROWS + 64 * TPW) * LDT * sizeof(float);
    if (lds > 64 * 1024) {   // above the default dynamic-LDS limit: raised once per process
        static bool raised = false;
        if (!raised) {
            TSM_HIP(tsm_allow_max_lds(reinterpret_cast<const void *>(ln_fwd_kernel<TPW>)));
            raised = true;
        }
    }
    hipLaunchKernelGGL((ln_fwd_kernel<TPW>), dim3((unsigned)ceil_div(g.M, LN_ROWS)), dim3(NT), lds, stream, g);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

int ln_fwd(const LnFwdArgs &g, hipStream_t stream) {
    const int64_t per = ceil_div(ceil_div(g.O, 16), 4);   // tiles per wave
    if (per <= 1) return ln_fwd_launch<1>(g, stream);
    if (per <= 2) return ln_fwd_launch<2>(g, stream);
    if (per <= 4) return ln_fwd_launch<4>(g, stream);
    return ln_fwd_launch<8>(g, stream);
}

// the row kernel on layer l's block: da (in d_acts) -> dy in place; n_split >= 1: the slabs' gamma / beta gradients too
int ln_bwd_rows(const tsm_mlp_desc *d, int l, const float *params, const float *saved, float *d_acts, int64_t B,
                const int64_t *p_off, const int64_t *a_off, const int64_t *s_off, int32_t n_split, float *slabs,
                int64_t slab_stride, hipStream_t stream) {
    const int64_t K = d->dims[l], O = d->dims[l + 1];
    LnBwdArgs g{};
    g.da = d_acts + a_off[l]; g.dy = d_acts + a_off[l];
    g.xhat = saved + s_off[l]; g.rstd = saved + s_off[l] + B * O;
    g.gamma = params + p_off[l] + O * K + O; g.beta = g.gamma + O;
    g.B = B; g.O = (int32_t)O; g.act = d->act;
    g.with_params = n_split >= 1;
    g.k_per = g.with_params ? ceil_div(ceil_div(B, n_split), BK) * BK : LN_ROWS;   // slab rows as tsm_mlp_backward
    g.slabs = slabs; g.slab_stride = slab_stride; g.g_off = p_off[l] + O * K + O; g.be_off = g.g_off + O;
    const unsigned grid = g.with_params ? (unsigned)n_split : (unsigned)ceil_div(B, LN_ROWS);
    hipLaunchKernelGGL(ln_bwd_rows_kernel, dim3(grid), dim3(LN_BWD_WAVES * kWave), 0, stream, g);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

}  // namespace

TSM_EXPORT int tsm_mlp_ln_param_count(const tsm_mlp_desc *d, int64_t *n_param) {
    if (int rc = ln_check(d, "tsm_mlp_ln_param_count")) return rc;
    TSM_REQUIRE(n_param, "tsm_mlp_ln_param_count: null pointer");
    int64_t p_off[TSM_MLP_MAX_LAYERS], a_off[TSM_MLP_MAX_LAYERS], s_off[TSM_MLP_MAX_LAYERS];
    *n_param = ln_offsets(d, 0, p_off, a_off, s_off);
    return TSM_OK;
}

TSM_EXPORT int tsm_mlp_ln_save_elems(const tsm_mlp_desc *d, int64_t B, int64_t *n_save) {
    if (int rc = ln_check(d, "tsm_mlp_ln_save_elems")) return rc;
    TSM_REQUIRE(B >= 0, "tsm_mlp_ln_save_elems: negative batch");
    TSM_REQUIRE(n_save, "tsm_mlp_ln_save_elems: null pointer");
    int64_t n = 0;
    for (int l = 1; l < d->n_layers; ++l) n += B * d->dims[l] + B;
    *n_save = n;
    return TSM_OK;
}

TSM_EXPORT int tsm_mlp_ln_forward(const tsm_mlp_desc *d, float eps, const float *params, const float *x, int64_t B, float *acts,
                                  float *saved, void *stream) {
    if (int rc = ln_check(d, "tsm_mlp_ln_forward")) return rc;
    TSM_REQUIRE(eps > 0.f && eps < 1e30f, "tsm_mlp_ln_forward: eps must be positive and finite");
    TSM_REQUIRE(B >= 0, "tsm_mlp_ln_forward: negative batch");
    if (B == 0) return TSM_OK;
    TSM_REQUIRE(params && x && acts, "tsm_mlp_ln_forward: null pointer");
    TSM_REQUIRE(ceil_div(B, 64) <= 65535, "tsm_mlp_ln_forward: batch %lld too large for one launch (max %d rows)", (long long)B,
                65535 * 64);
    const int L = d->n_layers;
    int64_t p_off[TSM_MLP_MAX_LAYERS], a_off[TSM_MLP_MAX_LAYERS], s_off[TSM_MLP_MAX_LAYERS];
    ln_offsets(d, B, p_off, a_off, s_off);
    const float *in = x;
    for (int l = 0; l < L; ++l) {
        const int32_t K = d->dims[l], O = d->dims[l + 1];
        const float *W = params + p_off[l], *b = W + (int64_t)O * K;
        float *out = acts + a_off[l];
        if (l + 1 < L) {
            LnFwdArgs g{};
            g.X = in; g.W = W; g.bias = b; g.gamma = b + O; g.beta = b + 2 * O;
            g.M = B; g.K = K; g.O = O; g.act = d->act; g.eps = eps; g.out = out;
            g.xhat = saved ? saved + s_off[l] : nullptr;
            g.rstd = saved ? saved + s_off[l] + B * O : nullptr;
            if (int rc = ln_fwd(g, tsm_stream(stream))) return rc;
        } else if (int rc = tsm_dense_linear(in, K, W, b, B, K, O, out, stream)) {
            return rc;
        }
        in = out;
    }
    return TSM_OK;
}

TSM_EXPORT int tsm_mlp_ln_backward(const tsm_mlp_desc *d, const float *params, const float *x, int64_t B, const float *acts,
                                   const float *saved, const float *d_out, float *d_acts, int32_t n_split, float *slabs,
                                   int64_t slab_stride, void *stream) {
    if (int rc = ln_check(d, "tsm_mlp_ln_backward")) return rc;
    TSM_REQUIRE(B >= 1, "tsm_mlp_ln_backward: batch must be >= 1");
    TSM_REQUIRE(n_split >= 1 && n_split <= 65535, "tsm_mlp_ln_backward: n_split out of range");
    TSM_REQUIRE(params && x && acts && d_out && slabs, "tsm_mlp_ln_backward: null pointer");
    TSM_REQUIRE(d->n_layers == 1 || (d_acts && saved), "tsm_mlp_ln_backward: d_acts workspace and saved required for n_layers > 1");
    TSM_REQUIRE(ceil_div(B, 64) <= 65535, "tsm_mlp_ln_backward: batch too large for one launch");
    const int L = d->n_layers;
    int64_t p_off[TSM_MLP_MAX_LAYERS], a_off[TSM_MLP_MAX_LAYERS], s_off[TSM_MLP_MAX_LAYERS];
    const int64_t n_param = ln_offsets(d, B, p_off, a_off, s_off);
    TSM_REQUIRE(slab_stride == 0 || slab_stride >= n_param, "tsm_mlp_ln_backward: slab_stride smaller than the parameter count");
    if (slab_stride == 0) slab_stride = n_param;
    const float *dz = d_out;   // gradient w.r.t. layer l's Linear output: d_out, then the row kernel's dy
    for (int l = L - 1; l >= 0; --l) {
        const int32_t K = d->dims[l], O = d->dims[l + 1];
        const float *in = l == 0 ? x : acts + a_off[l - 1];
        const float *W = params + p_off[l];
        if (int rc = tsm_dense_wgrad(dz, in, K, B, O, K, n_split, slabs, slab_stride, p_off[l], p_off[l] + (int64_t)O * K, stream))
            return rc;
        if (l > 0) {
            float *da = d_acts + a_off[l - 1];
            if (int rc = tsm_dense_dgrad(dz, W, B, O, K, da, K, stream)) return rc;
            if (int rc = ln_bwd_rows(d, l - 1, params, saved, d_acts, B, p_off, a_off, s_off, n_split, slabs, slab_stride,
                                     tsm_stream(stream)))
                return rc;
            dz = da;
        }
    }
    return TSM_OK;
}

TSM_EXPORT int tsm_mlp_ln_input_grad(const tsm_mlp_desc *d, const float *params, const float *x, int64_t B, const float *acts,
                                     const float *saved, const float *d_out, float *d_acts, int32_t col0, int32_t n_col,
                                     float *dx, int64_t ldx, void *stream) {
    if (int rc = ln_check(d, "tsm_mlp_ln_input_grad")) return rc;
    TSM_REQUIRE(B >= 1, "tsm_mlp_ln_input_grad: batch must be >= 1");
    TSM_REQUIRE(col0 >= 0 && n_col >= 1 && (int64_t)col0 + n_col <= d->dims[0],
                "tsm_mlp_ln_input_grad: columns [%d, %d + %d) leave the input width %d", col0, col0, n_col, d->dims[0]);
    TSM_REQUIRE(ldx >= n_col, "tsm_mlp_ln_input_grad: ldx = %lld smaller than n_col = %d", (long long)ldx, n_col);
    TSM_REQUIRE(params && x && acts && d_out && dx, "tsm_mlp_ln_input_grad: null pointer");
    TSM_REQUIRE(d->n_layers == 1 || (d_acts && saved), "tsm_mlp_ln_input_grad: d_acts workspace and saved required for n_layers > 1");
    TSM_REQUIRE(ceil_div(B, 64) <= 65535, "tsm_mlp_ln_input_grad: batch too large for one launch");
    const int L = d->n_layers;
    int64_t p_off[TSM_MLP_MAX_LAYERS], a_off[TSM_MLP_MAX_LAYERS], s_off[TSM_MLP_MAX_LAYERS];
    ln_offsets(d, B, p_off, a_off, s_off);
    const float *dz = d_out;
    for (int l = L - 1; l >= 0; --l) {
        const int32_t K = d->dims[l], O = d->dims[l + 1];
        const float *W = params + p_off[l];
        if (l > 0) {
            float *da = d_acts + a_off[l - 1];
            if (int rc = tsm_dense_dgrad(dz, W, B, O, K, da, K, stream)) return rc;
            if (int rc = ln_bwd_rows(d, l - 1, params, saved, d_acts, B, p_off, a_off, s_off, 0, nullptr, 0, tsm_stream(stream)))
                return rc;
            dz = da;
        } else if (int rc = tsm_dense_dgrad_window(dz, W + col0, K, B, O, n_col, dx, ldx, stream)) {   // the window of W_0's columns
            return rc;
        }
    }
    return TSM_OK;
}
