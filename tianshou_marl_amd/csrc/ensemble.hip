// ensemble.hip -- an ensemble of E fully-connected networks of one shape as ONE grouped launch per layer and role.
//
// Replaces, in /root/reference/tianshou:
//   EnsembleLinear.forward (torch.matmul(x, weight [E, in, out]) + bias_weights [E, 1, out])   utils/net/common.py:522-554
//   the stack ContinuousCritic(Net(linear_layer=EnsembleLinear), linear_layer=EnsembleLinear)    utils/net/continuous.py:102-175
//   and `loss.backward()` through it                                                          algorithm/modelfree/redq.py:274-289
//
// The grouped form of csrc/dense.hip's three GEMM roles on the same f32-input MFMA (v_mfma_f32_16x16x4_f32: exact f32 products,
// so the 1e-5 bar holds), the same 64x64 output tile per 4-wave workgroup, the same double-buffered 64x16 LDS tiles
// (gemm_tile_dev.h).  The ensemble member is a grid dimension: blockIdx.z = member (forward, dgrad) or member * n_split + slab
// (wgrad).  Every operand carries a member stride; a stride of 0 is an operand all members share (the first layer's input).
//
// Parameter vector layout = the reference's `parameters()` order, per layer: weight [E][in][out], then bias_weights [E][1][out].
// A member's weight is k-major for the forward product (W[k][n], contiguous along the output), the other way round from
// dense.hip's [out][in], so the operand roles of the forward and dgrad products swap relative to dense.hip:
//   forward   Y_e[B,O]  = act(X_e[B,K] . W_e[K,O] + b_e)              A row-major, B k-major
//   dgrad     dX_e[B,K] = (dZ_e[B,O] . W_e[K,O]^T) * act'(X_e)        A row-major, B row-major ([N = K][k = O])
//   wgrad     dW_e[K,O] = X_e^T . dZ_e,  db_e[O] = column sums of dZ_e A k-major + a virtual ones row (row K = db), B k-major,
//             split over the batch into `n_split` slabs (deterministic; tsm_adam_step sums the slabs)
//   input gradient's last product   dx[B, n_col] = sum_e dZ0_e[B,O] . W0_e[col0 : col0 + n_col, :O]^T: one workgroup walks
//             the members e = 0 .. E - 1 in order as the outer part of its k loop over E * O -- one writer per element, no atomics.
// Every sum has a fixed order, so two runs give the same bits.
#include "common.h"
#include "gemm_tile_dev.h"

namespace {

enum { EPI_FWD = 0, EPI_DGRAD = 1, EPI_WGRAD = 2 };

struct EnsGemmArgs {
    const float *A; int64_t lda, a_ms;   // row-major: A[m*lda + k]; k-major: A[k*lda + m];  *_ms: member stride (0: shared)
    const float *B; int64_t ldb, b_ms;   // row-major: B[n*ldb + k]; k-major: B[k*ldb + n]
    int64_t M, N, K;                     // M includes the virtual ones row for wgrad;  K: the k extent of ONE member
    int64_t k_per_split;
    int32_t n_split;                     // wgrad: blockIdx.z = member * n_split + slab;  else 1
    int32_t n_inner;                     // members summed inside the k loop, in order (the input gradient's last product);  else 1
    float *C; int64_t ldc, c_ms;         // fwd / dgrad output
    const float *bias; int64_t bias_ms;  // fwd
    const float *X; int64_t ldx, x_ms;   // dgrad: layer input (activation output of the previous layer)
    int act;                             // 0 none, 1 relu, 2 tanh (fwd: applied; dgrad: derivative w.r.t. X)
    int64_t slab_stride, w_off, b_off;   // wgrad: member e's dW at w_off + e * (M - 1) * N, its db at b_off + e * N
};

template <bool A_KMAJOR, bool B_KMAJOR, int EPI>
__global__ __launch_bounds__(NT) void ens_gemm_kernel(EnsGemmArgs g) {
    constexpr int kTile = (BM + BN) * LDT;  // one A tile + one B tile
    __shared__ __attribute__((aligned(16))) float lds[2 * kTile];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int64_t m0 = (int64_t)blockIdx.y * BM, n0 = (int64_t)blockIdx.x * BN;
    const int member = (int)blockIdx.z / g.n_split, slab = (int)blockIdx.z % g.n_split;
    const int64_t kbeg = (int64_t)slab * g.k_per_split;
    const int64_t kend = kbeg + g.k_per_split < g.K ? kbeg + g.k_per_split : g.K;
    const int per_member = kend > kbeg ? (int)((kend - kbeg + BK - 1) / BK) : 0;   // k tiles of one member
    const int n_iter = per_member * g.n_inner;
    const int64_t ones_m = EPI == EPI_WGRAD ? g.M - 1 : -1;

    f4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};

    const auto al16 = [](const float *p, int64_t ld) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && (ld & 3) == 0; };
    float va[KS][4], vb[KS][4];
    int f_mem = 0, f_tile = 0;   // the (inner member, k tile) the next fetch stages: members outside, k inside
    auto fetch = [&]() {
        const float *Ap = g.A + (int64_t)(member + f_mem) * g.a_ms, *Bp = g.B + (int64_t)(member + f_mem) * g.b_ms;
        // workgroup-uniform "no edge, aligned" predicates of the two operands of this member (the k extent is checked per tile)
        const bool a_in = al16(Ap, g.lda) && m0 + BM <= (ones_m >= 0 ? ones_m : g.M);
        const bool b_in = al16(Bp, g.ldb) && n0 + BN <= g.N;
        const int64_t k0 = kbeg + (int64_t)f_tile * BK;
#pragma unroll
        for (int h = 0; h < KS; ++h) {
            const bool k_in = k0 + 16 * (h + 1) <= kend;
            if (A_KMAJOR) load_kmajor(Ap, g.lda, m0, g.M, k0 + 16 * h, kend, ones_m, va[h], tid, a_in && k_in);
            else load_rowmajor(Ap, g.lda, m0, g.M, k0 + 16 * h, kend, va[h], tid, a_in && k_in);
            if (B_KMAJOR) load_kmajor(Bp, g.ldb, n0, g.N, k0 + 16 * h, kend, -1, vb[h], tid, b_in && k_in);
            else load_rowmajor(Bp, g.ldb, n0, g.N, k0 + 16 * h, kend, vb[h], tid, b_in && k_in);
        }
        if (++f_tile == per_member) { f_tile = 0; ++f_mem; }
    };
    auto commit = [&](int buf) {
        float *at = lds + buf * kTile, *bt = at + BM * LDT;
#pragma unroll
        for (int h = 0; h < KS; ++h) {
            if (A_KMAJOR) store_kmajor(at, va[h], tid, 16 * h); else store_rowmajor(at, va[h], tid, 16 * h);
            if (B_KMAJOR) store_kmajor(bt, vb[h], tid, 16 * h); else store_rowmajor(bt, vb[h], tid, 16 * h);
        }
    };

    int buf = 0;
    if (n_iter > 0) {
        fetch();
        commit(0);
    }
    __syncthreads();
    for (int it = 0; it < n_iter; ++it) {
        const bool more = it + 1 < n_iter;
        if (more) fetch();  // global loads of the next tile fly while this one is multiplied
        const float *a_t = lds + buf * kTile + (wm * 32 + (lane & 15)) * LDT + (lane >> 4);
        const float *b_t = lds + buf * kTile + BM * LDT + (wn * 32 + (lane & 15)) * LDT + (lane >> 4);
#pragma unroll
        for (int kk = 0; kk < BK; kk += 4) {
            const float a0 = a_t[kk], a1 = a_t[16 * LDT + kk];
            const float b0 = b_t[kk], b1 = b_t[16 * LDT + kk];
            acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        if (more) commit(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }

    // C fragment: register r of lane l holds C[(l >> 4) * 4 + r][l & 15]
    const int64_t e = member;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int64_t col = n0 + wn * 32 + j * 16 + (lane & 15);
            if (col >= g.N) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t row = m0 + wm * 32 + i * 16 + (lane >> 4) * 4 + r;
                if (row >= g.M) continue;
                float v = acc[i][j][r];
                if (EPI == EPI_FWD) {
                    g.C[e * g.c_ms + row * g.ldc + col] = act_fwd(v + g.bias[e * g.bias_ms + col], g.act);
                } else if (EPI == EPI_DGRAD) {
                    if (g.act) v *= act_bwd(g.X[e * g.x_ms + row * g.ldx + col], g.act);
                    g.C[e * g.c_ms + row * g.ldc + col] = v;
                } else {
                    float *dst = g.C + (int64_t)slab * g.slab_stride;
                    if (row == g.M - 1) dst[g.b_off + e * g.N + col] = v;                          // db_e[o]
                    else dst[g.w_off + e * (g.M - 1) * g.N + row * g.N + col] = v;                 // dW_e[k][o]
                }
            }
        }
}

int ens_check(const tsm_mlp_desc *d, int32_t E, const char *who) {
    if (int rc = check_desc(d, who)) return rc;
    TSM_REQUIRE(E >= 1 && E <= TSM_ENS_MAX_MEMBERS, "%s: ensemble size %d outside [1, %d]", who, E, TSM_ENS_MAX_MEMBERS);
    return TSM_OK;
}

// offsets of each layer's parameters (weight block; the bias block follows it) and of the block holding its OUTPUT
void ens_offsets(const tsm_mlp_desc *d, int64_t E, int64_t B, int64_t *p_off, int64_t *a_off) {
    int64_t po = 0, ao = 0;
    for (int l = 0; l < d->n_layers; ++l) {
        p_off[l] = po;
        a_off[l] = ao;
        po += E * ((int64_t)d->dims[l] * d->dims[l + 1] + d->dims[l + 1]);
        ao += E * B * d->dims[l + 1];
    }
}

// one dgrad launch of layer l > 0: d_acts block l - 1 <- (dz . W_l^T) * act'(acts block l - 1)
void ens_dgrad(const tsm_mlp_desc *d, int l, int64_t E, int64_t B, const float *W, const float *dz, const float *in, float *dx,
               hipStream_t s) {
    const int64_t K = d->dims[l], O = d->dims[l + 1];
    EnsGemmArgs g{};
    g.A = dz; g.lda = O; g.a_ms = B * O; g.B = W; g.ldb = O; g.b_ms = K * O; g.M = B; g.N = K; g.K = O; g.k_per_split = O;
    g.n_split = 1; g.n_inner = 1;
    g.C = dx; g.ldc = K; g.c_ms = B * K; g.X = in; g.ldx = K; g.x_ms = B * K; g.act = d->act;
    dim3 grid((unsigned)ceil_div(K, BN), (unsigned)ceil_div(B, BM), (unsigned)E);
    hipLaunchKernelGGL((ens_gemm_kernel<false, false, EPI_DGRAD>), grid, dim3(NT), 0, s, g);
}

}  // namespace

TSM_EXPORT int64_t tsm_ens_mlp_param_count(const tsm_mlp_desc *d, int32_t E) {
    if (ens_check(d, E, "tsm_ens_mlp_param_count") != TSM_OK) return -1;
    return (int64_t)E * tsm_mlp_param_count(d);
}

TSM_EXPORT int64_t tsm_ens_mlp_act_elems(const tsm_mlp_desc *d, int32_t E, int64_t B) {
    if (ens_check(d, E, "tsm_ens_mlp_act_elems") != TSM_OK || B < 0) return -1;
    return (int64_t)E * tsm_mlp_act_elems(d, B);
}

TSM_EXPORT int tsm_ens_mlp_forward(const tsm_mlp_desc *d, int32_t E, const float *params, const float *x, int64_t B,
                                   float *acts, void *stream) {
    if (int rc = ens_check(d, E, "tsm_ens_mlp_forward")) return rc;
    TSM_REQUIRE(B >= 0, "tsm_ens_mlp_forward: negative batch");
    if (B == 0) return TSM_OK;
    TSM_REQUIRE(params && x && acts, "tsm_ens_mlp_forward: null pointer");
    TSM_REQUIRE(ceil_div(B, BM) <= 65535, "tsm_ens_mlp_forward: batch %lld too large for one launch (max %d rows)",
                (long long)B, 65535 * BM);
    int64_t p_off[TSM_MLP_MAX_LAYERS], a_off[TSM_MLP_MAX_LAYERS];
    ens_offsets(d, E, B, p_off, a_off);
    for (int l = 0; l < d->n_layers; ++l) {
        const int64_t K = d->dims[l], O = d->dims[l + 1];
        EnsGemmArgs g{};
        g.A = l == 0 ? x : acts + a_off[l - 1]; g.lda = K; g.a_ms = l == 0 ? 0 : B * K;   // x is shared by all members
        g.B = params + p_off[l]; g.ldb = O; g.b_ms = K * O;
        g.M = B; g.N = O; g.K = K; g.k_per_split = K; g.n_split = 1; g.n_inner = 1;
        g.C = acts + a_off[l]; g.ldc = O; g.c_ms = B * O;
        g.bias = params + p_off[l] + (int64_t)E * K * O; g.bias_ms = O;
        g.act = l + 1 < d->n_layers ? d->act : 0;
        dim3 grid((unsigned)ceil_div(O, BN), (unsigned)ceil_div(B, BM), (unsigned)E);
        hipLaunchKernelGGL((ens_gemm_kernel<false, true, EPI_FWD>), grid, dim3(NT), 0, tsm_stream(stream), g);
        TSM_LAUNCH_CHECK();
    }
    return TSM_OK;
}

TSM_EXPORT int tsm_ens_mlp_backward(const tsm_mlp_desc *d, int32_t E, const float *params, const float *x, int64_t B,
                                    const float *acts, const float *d_out, float *d_acts, int32_t n_split, float *slabs,
                                    int64_t slab_stride, void *stream) {
    if (int rc = ens_check(d, E, "tsm_ens_mlp_backward")) return rc;
    TSM_REQUIRE(B >= 1, "tsm_ens_mlp_backward: batch must be >= 1");
    TSM_REQUIRE(n_split >= 1 && (int64_t)E * n_split <= 65535,
                "tsm_ens_mlp_backward: ensemble size %d x n_split %d outside [1, 65535] (one grid dimension)", E, n_split);
    TSM_REQUIRE(params && x && acts && d_out && slabs, "tsm_ens_mlp_backward: null pointer");
    TSM_REQUIRE(d->n_layers == 1 || d_acts, "tsm_ens_mlp_backward: d_acts workspace required for n_layers > 1");
    TSM_REQUIRE(ceil_div(B, BM) <= 65535, "tsm_ens_mlp_backward: batch too large for one launch");
    const int L = d->n_layers;
    const int64_t n_param = tsm_ens_mlp_param_count(d, E);
    TSM_REQUIRE(slab_stride == 0 || slab_stride >= n_param,
                "tsm_ens_mlp_backward: slab_stride smaller than the parameter count");
    if (slab_stride == 0) slab_stride = n_param;
    int64_t p_off[TSM_MLP_MAX_LAYERS], a_off[TSM_MLP_MAX_LAYERS];
    ens_offsets(d, E, B, p_off, a_off);
    // k range of the batch handled by one slab: a multiple of BK so that tiles never straddle two slabs
    const int64_t k_per = ceil_div(ceil_div(B, n_split), BK) * BK;
    const float *dz = d_out;  // gradient w.r.t. the pre-activation output of layer l (last layer is linear)
    for (int l = L - 1; l >= 0; --l) {
        const int64_t K = d->dims[l], O = d->dims[l + 1];
        const float *in = l == 0 ? x : acts + a_off[l - 1];
        {   // wgrad + bias grad into every slab
            EnsGemmArgs g{};
            g.A = in; g.lda = K; g.a_ms = l == 0 ? 0 : B * K; g.B = dz; g.ldb = O; g.b_ms = B * O;
            g.M = K + 1; g.N = O; g.K = B; g.k_per_split = k_per; g.n_split = n_split; g.n_inner = 1;
            g.C = slabs; g.slab_stride = slab_stride; g.w_off = p_off[l]; g.b_off = p_off[l] + (int64_t)E * K * O;
            dim3 grid((unsigned)ceil_div(O, BN), (unsigned)ceil_div(K + 1, BM), (unsigned)(E * n_split));
            hipLaunchKernelGGL((ens_gemm_kernel<true, true, EPI_WGRAD>), grid, dim3(NT), 0, tsm_stream(stream), g);
            TSM_LAUNCH_CHECK();
        }
        if (l > 0) {  // dgrad, multiplied by the derivative of the previous layer's activation
            float *dx = d_acts + a_off[l - 1];
            ens_dgrad(d, l, E, B, params + p_off[l], dz, in, dx, tsm_stream(stream));
            TSM_LAUNCH_CHECK();
            dz = dx;
        }
    }
    return TSM_OK;
}

TSM_EXPORT int tsm_ens_mlp_input_grad(const tsm_mlp_desc *d, int32_t E, const float *params, const float *x, int64_t B,
                                      const float *acts, const float *d_out, float *d_acts, int32_t col0, int32_t n_col,
                                      float *dx, int64_t ldx, void *stream) {
    if (int rc = ens_check(d, E, "tsm_ens_mlp_input_grad")) return rc;
    TSM_REQUIRE(B >= 1, "tsm_ens_mlp_input_grad: batch must be >= 1");
    TSM_REQUIRE(col0 >= 0 && n_col >= 1 && (int64_t)col0 + n_col <= d->dims[0],
                "tsm_ens_mlp_input_grad: columns [%d, %d + %d) leave the input width %d", col0, col0, n_col, d->dims[0]);
    TSM_REQUIRE(ldx >= n_col, "tsm_ens_mlp_input_grad: ldx = %lld smaller than n_col = %d", (long long)ldx, n_col);
    TSM_REQUIRE(params && x && acts && d_out && dx, "tsm_ens_mlp_input_grad: null pointer");
    TSM_REQUIRE(d->n_layers == 1 || d_acts, "tsm_ens_mlp_input_grad: d_acts workspace required for n_layers > 1");
    TSM_REQUIRE(ceil_div(B, BM) <= 65535, "tsm_ens_mlp_input_grad: batch too large for one launch");
    int64_t p_off[TSM_MLP_MAX_LAYERS], a_off[TSM_MLP_MAX_LAYERS];
    ens_offsets(d, E, B, p_off, a_off);
    const float *dz = d_out;
    for (int l = d->n_layers - 1; l > 0; --l) {   // as tsm_ens_mlp_backward, without its weight-gradient launches
        float *da = d_acts + a_off[l - 1];
        ens_dgrad(d, l, E, B, params + p_off[l], dz, acts + a_off[l - 1], da, tsm_stream(stream));
        TSM_LAUNCH_CHECK();
        dz = da;
    }
    // the window of W_0's input rows, summed over the members in order inside the k loop; no activation derivative: the input
    // is not an activation
    const int64_t K = d->dims[0], O = d->dims[1];
    EnsGemmArgs g{};
    g.A = dz; g.lda = O; g.a_ms = B * O; g.B = params + (int64_t)col0 * O; g.ldb = O; g.b_ms = K * O;
    g.M = B; g.N = n_col; g.K = O; g.k_per_split = O; g.n_split = 1; g.n_inner = E;
    g.C = dx; g.ldc = ldx; g.c_ms = 0; g.act = 0;
    dim3 grid((unsigned)ceil_div(n_col, BN), (unsigned)ceil_div(B, BM), 1);
    hipLaunchKernelGGL((ens_gemm_kernel<false, false, EPI_DGRAD>), grid, dim3(NT), 0, tsm_stream(stream), g);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}
