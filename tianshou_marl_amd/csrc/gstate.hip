// gstate.hip -- the learned global-state aggregations of GlobalStateConstructor, modes "attention" and "graph"
// (/root/reference/tianshou/algorithm/multiagent/ctde.py:268-280, 302-335): what lies BETWEEN their matrix products with
// weights.  The products themselves (in-projection, out-projection, output_proj, gnn_layer1, gnn_layer2) are csrc/dense.hip.
//
// attention  nn.MultiheadAttention(embed_dim = D, num_heads = 4, batch_first = True) on one joint row's N agents, then the
//            mean over the N query agents.  tsm_attn_pool_forward takes the in-projection's output qkv [B][N][3 D] and gives
//            ctx [B][D] = mean_n concat_h(softmax(Q_h K_h^T / sqrt(dh)) V_h)[n]: the mean commutes with the out-projection
//            (mean_n(W O_n + b) = W mean_n O_n + b), so that product runs on B rows, not B N.
// graph      mean_n(W2 (A^ relu(h))_n + b2) = W2 (sum_m c_m relu(h_m)) + b2 with c_m = (1 / N) sum_n A^[n][m], A^ the
//            row-normalised adjacency: tsm_agent_pool_forward is that weighted sum over the agents.
//
// A VALU formulation: with N <= 8 a head's score tile is at most 8 x 8 and a row holds 4 of them, far below one 16x16x4 MFMA
// tile per wave, and every fold (the dot products over dh, the softmax over j, the sums over agents) runs inside ONE lane in
// index order.  No cross-lane reduction, no atomics: two runs give the same bits.  One wave serves one joint row; its qkv
// row is staged once into LDS with 16-B loads.
#include "common.h"

namespace {
constexpr int kHeads = TSM_GSTATE_HEADS;
constexpr int kRows = TSM_GSTATE_ROWS_PER_BLOCK;   // joint rows per workgroup: one wave each
constexpr int kThreads = kRows * kWave;
constexpr int kPoolThreads = 256;

// floats of LDS one wave needs (a multiple of 4: every wave's base stays 16-B aligned)
__host__ __device__ constexpr int attn_fwd_floats(int N, int D) { return N * 3 * D + kHeads * N * N + kHeads * N; }
__host__ __device__ constexpr int attn_bwd_floats(int N, int D) {
    return N * 3 * D + 2 * kHeads * N * N + 2 * kHeads * N + D;
}

// Stage n floats (n % 4 == 0, both bases 16-B aligned) of this wave's row into LDS; `ok` false: zeros.
__device__ __forceinline__ void stage_row(float *dst, const float *__restrict__ src, int n, int lane, bool ok) {
    for (int e = 4 * lane; e < n; e += 4 * kWave) {
        const float4 v = ok ? ld4(src + e) : make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4 *>(dst + e) = v;
    }
}

// qkv [B][N][3 D] -> ctx [B][D], P [B][4][N][N]
__global__ __launch_bounds__(kThreads) void attn_pool_forward_kernel(const float *__restrict__ qkv, int64_t B, int32_t N,
                                                                     int32_t D, float *__restrict__ ctx,
                                                                     float *__restrict__ P) {
    extern __shared__ __align__(16) float lds[];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t b = (int64_t)blockIdx.x * kRows + w;
    const bool ok = b < B;
    const int dh = D / kHeads, row = N * 3 * D, NN = N * N;
    float *x = lds + (size_t)w * attn_fwd_floats(N, D);   // [N][3 D]: Q | K | V per agent
    float *p = x + row;                                    // [4][N][N]
    float *pbar = p + kHeads * NN;                         // [4][N]: sum_i P[h][i][j]
    stage_row(x, qkv + (ok ? b : 0) * row, row, lane, ok);
    __syncthreads();
    // lane (h, i): the N scores of query i in head h, their softmax with the maximum subtracted
    if (lane < kHeads * N) {
        const int h = lane / N, i = lane - h * N;
        const float scale = 1.f / sqrtf((float)dh);
        const float *q = x + i * 3 * D + h * dh;
        float s[TSM_GSTATE_MAX_AGENTS];
        float mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < TSM_GSTATE_MAX_AGENTS; ++j) {
            if (j < N) {
                const float *k = x + j * 3 * D + D + h * dh;
                float acc = 0.f;
                for (int t = 0; t < dh; ++t) acc = fmaf(q[t] * scale, k[t], acc);
                s[j] = acc;
                mx = fmaxf(mx, acc);
            } else {
                s[j] = 0.f;
            }
        }
        float den = 0.f;
#pragma unroll
        for (int j = 0; j < TSM_GSTATE_MAX_AGENTS; ++j)
            if (j < N) {
                s[j] = expf(s[j] - mx);
                den += s[j];
            }
        const float inv = 1.f / den;
#pragma unroll
        for (int j = 0; j < TSM_GSTATE_MAX_AGENTS; ++j)
            if (j < N) p[(h * N + i) * N + j] = s[j] * inv;
    }
    __syncthreads();
    if (lane < kHeads * N) {   // lane (h, j): the column sum over the queries, in order
        const int h = lane / N, j = lane - h * N;
        float acc = 0.f;
        for (int i = 0; i < N; ++i) acc += p[(h * N + i) * N + j];
        pbar[lane] = acc;
    }
    if (ok)
        for (int e = lane; e < kHeads * NN; e += kWave) P[b * (kHeads * NN) + e] = p[e];
    __syncthreads();
    const float inv_n = 1.f / (float)N;
    for (int d = lane; d < D; d += kWave) {   // ctx[d] = (1 / N) sum_j pbar[h][j] V[j][d]
        const int h = d / dh;
        float acc = 0.f;
        for (int j = 0; j < N; ++j) acc = fmaf(pbar[h * N + j], x[j * 3 * D + 2 * D + d], acc);
        if (ok) ctx[b * D + d] = acc * inv_n;
    }
}

// d_ctx [B][D], qkv, P -> d_qkv [B][N][3 D]
__global__ __launch_bounds__(kThreads) void attn_pool_backward_kernel(const float *__restrict__ d_ctx,
                                                                      const float *__restrict__ qkv,
                                                                      const float *__restrict__ P, int64_t B, int32_t N,
                                                                      int32_t D, float *__restrict__ d_qkv) {
    extern __shared__ __align__(16) float lds[];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t b = (int64_t)blockIdx.x * kRows + w;
    const bool ok = b < B;
    const int dh = D / kHeads, row = N * 3 * D, NN = N * N;
    float *x = lds + (size_t)w * attn_bwd_floats(N, D);   // [N][3 D]
    float *p = x + row;                                    // [4][N][N]
    float *ds = p + kHeads * NN;                           // [4][N][N]: d S, the 1 / sqrt(dh) folded in
    float *g = ds + kHeads * NN;                           // [4][N]: d P[h][.][j], the same for every query
    float *pbar = g + kHeads * N;                          // [4][N]
    float *dc = pbar + kHeads * N;                         // [D]: d_ctx / N
    const float inv_n = 1.f / (float)N;
    stage_row(x, qkv + (ok ? b : 0) * row, row, lane, ok);
    for (int e = lane; e < kHeads * NN; e += kWave) p[e] = ok ? P[b * (kHeads * NN) + e] : 0.f;
    for (int d = lane; d < D; d += kWave) dc[d] = ok ? d_ctx[b * D + d] * inv_n : 0.f;
    __syncthreads();
    // ctx = (1 / N) sum_i P_i V: every query's d O is d_ctx / N, so d P[h][i][j] = sum_t dc[h dh + t] V[j][h dh + t] for all i
    if (lane < kHeads * N) {
        const int h = lane / N, j = lane - h * N;
        const float *v = x + j * 3 * D + 2 * D + h * dh;
        float acc = 0.f, col = 0.f;
        for (int t = 0; t < dh; ++t) acc = fmaf(dc[h * dh + t], v[t], acc);
        for (int i = 0; i < N; ++i) col += p[(h * N + i) * N + j];
        g[lane] = acc;
        pbar[lane] = col;
    }
    __syncthreads();
    if (lane < kHeads * N) {   // lane (h, i): the softmax Jacobian, d S = P (d P - sum_j P d P)
        const int h = lane / N, i = lane - h * N;
        const float scale = 1.f / sqrtf((float)dh);
        const float *pr = p + (h * N + i) * N;
        float dot = 0.f;
        for (int j = 0; j < N; ++j) dot = fmaf(pr[j], g[h * N + j], dot);
        for (int j = 0; j < N; ++j) ds[(h * N + i) * N + j] = pr[j] * (g[h * N + j] - dot) * scale;
    }
    __syncthreads();
    if (!ok) return;
    float *out = d_qkv + b * row;
    for (int e = lane; e < row; e += kWave) {
        const int n = e / (3 * D), c = e - n * 3 * D;
        const int part = c / D, d = c - part * D, h = d / dh;
        float acc = 0.f;
        if (part == 0) {          // d Q[n][d] = sum_j d S[h][n][j] K[j][d]
            for (int j = 0; j < N; ++j) acc = fmaf(ds[(h * N + n) * N + j], x[j * 3 * D + D + d], acc);
        } else if (part == 1) {   // d K[n][d] = sum_i d S[h][i][n] Q[i][d]
            for (int i = 0; i < N; ++i) acc = fmaf(ds[(h * N + i) * N + n], x[i * 3 * D + d], acc);
        } else {                  // d V[n][d] = (d_ctx[d] / N) sum_i P[h][i][n]
            acc = dc[d] * pbar[h * N + n];
        }
        out[e] = acc;
    }
}

// out[b][k] = sum_n c[n] f(h[b][n][k]), n in order; f = relu or the identity
__global__ __launch_bounds__(kPoolThreads) void agent_pool_forward_kernel(const float *__restrict__ h,
                                                                          const float *__restrict__ c, int64_t B, int32_t N,
                                                                          int32_t H, int relu, float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kPoolThreads + threadIdx.x;
    if (i >= B * H) return;
    const int64_t b = i / H;
    const int32_t k = (int32_t)(i - b * H);
    float acc = 0.f;
    for (int n = 0; n < N; ++n) {
        float v = h[(b * N + n) * H + k];
        if (relu) v = fmaxf(v, 0.f);
        acc = fmaf(c[n], v, acc);
    }
    out[i] = acc;
}

// d_h[b][n][k] = c[n] d[b][k] (relu: where h[b][n][k] > 0, else 0)
__global__ __launch_bounds__(kPoolThreads) void agent_pool_backward_kernel(const float *__restrict__ d,
                                                                           const float *__restrict__ c,
                                                                           const float *__restrict__ h, int64_t B, int32_t N,
                                                                           int32_t H, float *__restrict__ d_h) {
    const int64_t i = (int64_t)blockIdx.x * kPoolThreads + threadIdx.x;   // over B N H, output order
    if (i >= B * N * H) return;
    const int64_t bn = i / H;
    const int32_t k = (int32_t)(i - bn * H);
    const int64_t b = bn / N;
    const int32_t n = (int32_t)(bn - b * N);
    const float v = c[n] * d[b * H + k];
    d_h[i] = (h && !(h[i] > 0.f)) ? 0.f : v;
}

int check_shape(const char *who, int64_t B, int32_t N, int32_t D) {
    TSM_REQUIRE(N >= 1 && N <= TSM_GSTATE_MAX_AGENTS, "%s: n_agents = %d; the kernels serve 1 to %d agents", who, N,
                TSM_GSTATE_MAX_AGENTS);
    TSM_REQUIRE(D >= kHeads && D <= TSM_GSTATE_MAX_DIM && D % kHeads == 0,
                "%s: obs_dim = %d; the kernels serve multiples of %d from %d to %d (4 heads of at most 64)", who, D, kHeads,
                kHeads, TSM_GSTATE_MAX_DIM);
    TSM_REQUIRE(B >= 1 && ceil_div(B, kRows) <= 0x7fffffffLL, "%s: B = %lld rows; at least 1 and at most %lld", who,
                (long long)B, (long long)kRows * 0x7fffffffLL);
    return TSM_OK;
}

int check_pool(const char *who, int64_t B, int32_t N, int32_t H, bool per_agent) {
    TSM_REQUIRE(N >= 1 && N <= TSM_GSTATE_MAX_AGENTS, "%s: n_agents = %d; the kernels serve 1 to %d agents", who, N,
                TSM_GSTATE_MAX_AGENTS);
    TSM_REQUIRE(H >= 1, "%s: H = %d; at least 1", who, H);
    const int64_t per_row = (int64_t)H * (per_agent ? N : 1);   // one thread per element, 2^31 - 1 workgroups at most
    TSM_REQUIRE(B >= 1 && B <= 0x7fffffffLL * kPoolThreads / per_row, "%s: B = %lld rows of %lld elements; at least 1 and at most %lld",
                who, (long long)B, (long long)per_row, (long long)(0x7fffffffLL * kPoolThreads / per_row));
    return TSM_OK;
}
}  // namespace

TSM_EXPORT int tsm_gstate_check(int32_t n_agents, int32_t obs_dim) { return check_shape("tsm_gstate_check", 1, n_agents, obs_dim); }

TSM_EXPORT int tsm_attn_pool_forward(const float *qkv, int64_t B, int32_t n_agents, int32_t D, float *ctx, float *P,
                                     void *stream) {
    if (int rc = check_shape("tsm_attn_pool_forward", B, n_agents, D)) return rc;
    TSM_REQUIRE(qkv && ctx && P, "tsm_attn_pool_forward: null pointer");
    TSM_REQUIRE(reinterpret_cast<uintptr_t>(qkv) % 16 == 0, "tsm_attn_pool_forward: qkv must be 16-byte aligned");
    const size_t shmem = (size_t)kRows * attn_fwd_floats(n_agents, D) * sizeof(float);
    static bool attr_set = false;
    if (!attr_set) {
        TSM_HIP(tsm_allow_max_lds(reinterpret_cast<const void *>(attn_pool_forward_kernel)));
        attr_set = true;
    }
    hipLaunchKernelGGL(attn_pool_forward_kernel, dim3((unsigned)ceil_div(B, kRows)), dim3(kThreads), shmem, tsm_stream(stream),
                       qkv, B, n_agents, D, ctx, P);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_attn_pool_backward(const float *d_ctx, const float *qkv, const float *P, int64_t B, int32_t n_agents,
                                      int32_t D, float *d_qkv, void *stream) {
    if (int rc = check_shape("tsm_attn_pool_backward", B, n_agents, D)) return rc;
    TSM_REQUIRE(d_ctx && qkv && P && d_qkv, "tsm_attn_pool_backward: null pointer");
    TSM_REQUIRE(reinterpret_cast<uintptr_t>(qkv) % 16 == 0, "tsm_attn_pool_backward: qkv must be 16-byte aligned");
    const size_t shmem = (size_t)kRows * attn_bwd_floats(n_agents, D) * sizeof(float);
    static bool attr_set = false;
    if (!attr_set) {
        TSM_HIP(tsm_allow_max_lds(reinterpret_cast<const void *>(attn_pool_backward_kernel)));
        attr_set = true;
    }
    hipLaunchKernelGGL(attn_pool_backward_kernel, dim3((unsigned)ceil_div(B, kRows)), dim3(kThreads), shmem,
                       tsm_stream(stream), d_ctx, qkv, P, B, n_agents, D, d_qkv);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_agent_pool_forward(const float *h, const float *c, int64_t B, int32_t n_agents, int32_t H, int32_t relu,
                                      float *out, void *stream) {
    if (int rc = check_pool("tsm_agent_pool_forward", B, n_agents, H, false)) return rc;
    TSM_REQUIRE(h && c && out, "tsm_agent_pool_forward: null pointer");
    hipLaunchKernelGGL(agent_pool_forward_kernel, dim3((unsigned)ceil_div(B * H, kPoolThreads)), dim3(kPoolThreads), 0,
                       tsm_stream(stream), h, c, B, n_agents, H, relu ? 1 : 0, out);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_agent_pool_backward(const float *d, const float *c, const float *h_relu, int64_t B, int32_t n_agents,
                                       int32_t H, float *d_h, void *stream) {
    if (int rc = check_pool("tsm_agent_pool_backward", B, n_agents, H, true)) return rc;
    TSM_REQUIRE(d && c && d_h, "tsm_agent_pool_backward: null pointer");
    hipLaunchKernelGGL(agent_pool_backward_kernel, dim3((unsigned)ceil_div(B * n_agents * H, kPoolThreads)),
                       dim3(kPoolThreads), 0, tsm_stream(stream), d, c, h_relu, B, n_agents, H, d_h);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}
