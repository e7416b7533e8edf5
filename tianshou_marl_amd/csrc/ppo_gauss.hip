// ppo_gauss.hip -- one PPO gradient step of a Gaussian policy over 64-64 nets in ONE launch: forward of actor and critic, the
// Gaussian policy head and the value head with their closed-form backward, and the backward of both nets down to per-workgroup
// gradient slabs.  Activations never leave the chip.
//
// Replaces, per minibatch, the chain GenericPPO._grad_step_gauss composes from the general kernels:
//   tsm_gather_rows (obs)                                                 csrc/vrb.hip
//   tsm_mlp_forward (actor), tsm_mlp_forward (critic): three GEMMs each    csrc/dense.hip
//   tsm_gauss_ppo_head                                                    csrc/gauss.hip       (ppo.py:182-196, 210-211)
//   tsm_ppo_loss_fwd_bwd, loss_kind 2                                     csrc/ppo_loss.hip    (ppo.py:198-208)
//   tsm_mlp_backward (actor), tsm_mlp_backward (critic)                   csrc/dense.hip
//   tsm_gauss_sigma_fold, tsm_u64_add                                     csrc/gauss.hip, csrc/adam.hip
// Adam (tsm_adam_step over the slabs) and tsm_ppo_finalize_many follow it, as they follow tsm_ppo_update_fused.
//
// Work split (ppo_update_split_kernel's, csrc/mlp_fused.hip).  Grid (n_blocks, 2): blockIdx.y = 0 carries the actor, 1 the critic --
// the loss is separable, so a workgroup holds ONE net.  Workgroup (b, net) of four waves walks the 16-row tiles b, b + n_blocks, ...;
// wave w owns hidden columns [16 w, 16 w + 16) of both hidden layers: their forward chains, their input-gradient chains and the
// weight-gradient accumulators of those rows of W1 / W2 (and those columns of W3), which stay in registers over all tiles --
// 4 NJ + 16 + 4 accumulator registers per lane -- and are stored once, behind the last tile.
//
// Slabs.  Slab b is one row of slab_stride floats in the flat vector's order.  Workgroup (b, 0) writes every actor column of it
// (w0 b0 w1 b1 w2 b2 and, when sigma is state-independent, sigma_param), workgroup (b, 1) every critic column: each column of the
// parameter range has exactly one writer, none is written as filler, and the pad [n_param, slab_stride) is never touched.
//
// LDS of one net (floats; ld1 = 16 NJ + 2 with NJ = ceil(D / 16), ldh = 66, ldo = 18: row strides of 2 x odd dwords, the pads of
// the [lane & 15][lane >> 4] operand reads; 54.2 KB at D = 18, 64.4 KB at D = 64 -- two workgroups per CU at every D):
//   W1 [64][ld1] | W2 [64][ldh] | W3 [16][ldh] (rows past the head's width zero; the critic's has one row) | B1 B2 [64] | B3 [16]
//   SG [16] sigma_param | X [16][ld1] | H1 H2 [16][ldh] | OUT [16][ldo] raw outputs (critic: V in column 0) | D3 [16][ldo]
//   d loss / d raw (columns past the head's width stay zero) | D2 D1 [16][ldh] | f64: HC the head's constants, COL [16][16]
//   d loss / d sigma_param per (row, component), OBJ ENT [16] the rows' loss terms (critic: OBJ = the value loss)
// Weights are staged from the flat vector with tsm_stage_padded (there is no parameter image for this net).
//
// Per tile (a barrier behind each phase):
//   0. the tile's rows, gathered through perm into registers during the previous tile's backward, go to X
//   1. 2. hidden layers: one v_mfma_f32_16x16x4_f32 chain per wave over the zero-padded k range in ascending steps of 4, bias and
//      activation behind the chain -- dense.hip's order per output element, so OUT carries tsm_mlp_forward's bits
//   3. output layer on wave 0 (<= 16 columns: one block)
//   4. head.  Actor: gauss_dev.h's arithmetic in f64 on 16 rows x 16 lanes (component k in lane k; gu_actor_head, out of line so
//      that device libm stays out of the tile loop's register budget) -> D3, COL, OBJ, ENT.  Groups of 16 lanes give the sums of
//      tsm_gauss_ppo_head's groups of 8 bit for bit (the extra lanes add +0.0).  Critic: the value term of ppo_loss.hip in f32 on
//      one lane per row -> D3 column 0, OBJ.
//   5. dW3 += D3^T H2, dH2 = D3 W3 -> D2 through the activation's derivative (from the saved H2), db3; beside it single lanes fold
//      the tile's COL / OBJ / ENT rows, in row order, into their f64 running sums
//   6. dW2 += D2^T H1, db2, dH1 = D2 W2 -> D1        7. dW1 += D1^T X, db1
// Rows past M in a ragged last tile: X, the actions and D3 are exact zeros there, so they add +0.0 to every gradient and sum.
//
// Against the chain: raw outputs, V and the loss partials' per-row terms carry the same bits; the gradients do not (dense.hip sums
// a weight gradient over its row splits, this kernel over 16-row tiles) and the loss sums are grouped by tile instead of by 64 rows.
// No atomics: two runs give the same bits.
#include "common.h"
#include "gauss_dev.h"
#include "gemm_tile_dev.h"

namespace {

constexpr int kRows = 16, kHid = 64, kLdh = kHid + 2, kLdo = 18, kThreadsU = 256, kMaxOut = 16, kMaxNJ = 4;

struct GuLay {   // offsets in floats
    int ld1, W1, W2, W3, B1, B2, B3, SG, X, H1, H2, OUT, D3, D2, D1, HC, COL, OBJ, ENT, total;
    __host__ __device__ explicit GuLay(int NJ) {
        ld1 = 16 * NJ + 2;
        int o = 0;
        W1 = o; o += kHid * ld1;
        W2 = o; o += kHid * kLdh;
        W3 = o; o += kRows * kLdh;
        B1 = o; o += kHid;
        B2 = o; o += kHid;
        B3 = o; o += kMaxOut;
        SG = o; o += kMaxOut;
        X = o; o += kRows * ld1;
        H1 = o; o += kRows * kLdh;
        H2 = o; o += kRows * kLdh;
        OUT = o; o += kRows * kLdo;
        D3 = o; o += kRows * kLdo;
        D2 = o; o += kRows * kLdh;
        D1 = o; o += kRows * kLdh;
        o = (o + 1) & ~1;               // f64 cells: 8-byte alignment by index arithmetic off the 16-byte aligned base
        HC = o; o += 2 * 8;
        COL = o; o += 2 * kRows * kMaxOut;
        OBJ = o; o += 2 * kRows;
        ENT = o; o += 2 * kRows;
        total = o;
    }
};

struct GuHeadC {   // the actor head's constants, in LDS (8 doubles)
    double eps_clip, dual_clip, ent_coef, invM, mean, istd, max_action;
    int kind, flags;   // flags: bit 0 conditioned sigma, bit 1 unbounded; bits 8.. act_dim
};
static_assert(sizeof(GuHeadC) == 64, "HC is 16 floats");

struct GuArgs {
    const float *P;
    int D, Ad, out_w, cond, act_fn, unbounded;
    double max_action;
    const float *obs, *act, *logp_old, *adv, *ret, *v_old;
    const int64_t *perm;
    int64_t first, M;
    const float *adv_stats;
    double eps_clip, dual_clip, ent_coef;
    float eps_clip_f, vf_coef_f;
    int value_clip, adv_norm, kind;
    float *slabs;
    int64_t slab_stride;
    double *partial;
    int64_t *opt_step;
};

__device__ __forceinline__ f4 gu_mfma4(float a, float b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// acc[q] = sum_k A[i = lane & 15][k] B[k][j = lane & 15] for the output element (row (lane >> 4) * 4 + q, column lane & 15), k in
// ascending steps of 4: a / b point at this lane's element of k-step 0 (k = lane >> 4), sa / sb are the strides of one k.
template <int K>
__device__ __forceinline__ f4 gu_chain(const float *a, int sa, const float *b, int sb, f4 acc) {
#pragma unroll
    for (int k0 = 0; k0 < K; k0 += 4) acc = gu_mfma4(a[k0 * sa], b[k0 * sb], acc);
    return acc;
}

// sum over the 16 tile rows of one column, rows in increasing order, every read issued before the first addition
__device__ __forceinline__ float gu_column_sum(const float *col, int ld) {
    float v[kRows];
#pragma unroll
    for (int r = 0; r < kRows; ++r) v[r] = col[r * ld];
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < kRows; ++r) s += v[r];
    return s;
}

__device__ __forceinline__ float gu_act_grad(float g, float y, int act) { return act == 1 ? (y > 0.f ? g : 0.f) : g * act_bwd(y, act); }

// The policy head of one row on its group of 16 lanes (component k in lane k): gauss.hip's gauss_ppo_head_kernel per row, with
// the row's results left in LDS.  Every lane of the wave calls it (the sums over components are wave shuffles).
__device__ __noinline__ void gu_actor_head(const GuHeadC *hc, const float *raw, const float *sg, float a_f, float adv_f, float lpo_f,
                                           int k, bool live, float *d3_row, double *col_cell, double *obj_cell, double *ent_cell) {
    const int Ad = hc->flags >> 8;
    const bool in = k < Ad, cond = (hc->flags & 1) != 0;
    GaussLane o;
    gauss_lane(raw, cond ? raw + Ad : sg, cond, in, k, hc->max_action, (hc->flags & 2) != 0, o);
    double z;
    const double logp = gauss_row<16>(o, in ? a_f : 0.f, in, z);
    const double ent = group_sum<16>(in ? 0.5 + kLogSqrt2Pi + o.c : 0.0);
    const double A = ((double)adv_f - hc->mean) * hc->istd, lpo = (double)lpo_f;
    double obj, g_logp;   // d obj / d logp
    if (hc->kind == 1) {
        obj = logp * A;
        g_logp = A;
    } else {
        const double r = exp(logp - lpo), lo = 1.0 - hc->eps_clip, hi = 1.0 + hc->eps_clip;
        const double s1 = r * A, s2 = fmin(fmax(r, lo), hi) * A;
        const double g2 = (r >= lo && r <= hi) ? A : 0.0;   // clamp's backward: the closed interval
        double g_r;
        if (s1 < s2) { obj = s1; g_r = A; }
        else if (s2 < s1) { obj = s2; g_r = g2; }
        else { obj = s1; g_r = 0.5 * A + 0.5 * g2; }
        if (hc->dual_clip > 0.0 && A < 0.0) {   // ppo.py:190-194: max(min(s1, s2), c A) where A < 0
            const double cA = hc->dual_clip * A;
            if (cA > obj) { obj = cA; g_r = 0.0; }
            else if (cA == obj) g_r *= 0.5;
        }
        g_logp = g_r * r;
    }
    const double gl = -g_logp * hc->invM;
    const double dm = gl * (z / o.sigma) * o.dmu, dc = o.pass * (gl * (z * z - 1.0) - hc->ent_coef * hc->invM);
    const bool on = in && live;   // (selects, not products: a row past M may hold anything)
    if (in) {
        d3_row[k] = on ? (float)dm : 0.f;
        if (cond) d3_row[Ad + k] = on ? (float)dc : 0.f;
    }
    *col_cell = (on && !cond) ? dc : 0.0;
    if (k == 0) { *obj_cell = live ? obj : 0.0; *ent_cell = live ? ent : 0.0; }
}

template <int NJ, int NET>
__device__ __forceinline__ void gu_net(float *lds, const GuArgs &a) {
    constexpr int ld1 = 16 * NJ + 2, K1 = 16 * NJ;
    const GuLay ly(NJ);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c16 = lane & 15, kq = lane >> 4;
    const int D = a.D, Ad = a.Ad, act_fn = a.act_fn;
    const int ow = NET ? 1 : a.out_w;
    const int64_t M = a.M, n_tiles = (M + kRows - 1) / kRows;
    // this net's piece of the flat vector
    const int oB1 = kHid * D, oW2 = oB1 + kHid, oB2 = oW2 + kHid * kHid, oW3 = oB2 + kHid, oB3 = oW3 + ow * kHid;
    const int n_actor = kHid * D + 2 * kHid + kHid * kHid + a.out_w * kHid + a.out_w + (a.cond ? 0 : Ad);
    const float *P = a.P + (NET ? n_actor : 0);
    double *hc_d = reinterpret_cast<double *>(lds + ly.HC), *s_col = reinterpret_cast<double *>(lds + ly.COL);
    double *s_obj = reinterpret_cast<double *>(lds + ly.OBJ), *s_ent = reinterpret_cast<double *>(lds + ly.ENT);

    // ---- the tile's rows: gathered into registers one tile ahead ----
    float xr[NJ];
    float r_act, r_s0, r_s1;   // this lane's (row tid >> 4, component tid & 15): action | adv, logp_old (actor); returns, v_s_old (critic)
    auto prefetch = [&](int64_t t) {
        const int64_t row0 = t * kRows;
#pragma unroll
        for (int it = 0; it < NJ; ++it) {   // (unconditional loads at clamped, always-valid addresses + selects)
            const int e = tid + it * kThreadsU, r = e / D, c = e - r * D;
            const bool ok = e < kRows * D && row0 + r < M;
            const int64_t i = ok ? row0 + r : row0;
            const int64_t src = a.perm ? a.perm[i] : a.first + i;
            const float v = a.obs[src * D + c];
            xr[it] = ok ? v : 0.f;
        }
        const int r = tid >> 4, k = tid & 15;
        const bool live = row0 + r < M;
        const int64_t i = live ? row0 + r : row0;
        const int64_t src = a.perm ? a.perm[i] : a.first + i;
        r_act = 0.f;
        if (NET == 0) {
            const bool in = live && k < Ad;
            const float av = a.act[src * Ad + (k < Ad ? k : 0)];
            const float ad = a.adv[src], lp = (a.kind == 0 ? a.logp_old : a.adv)[src];   // (no branch around a load)
            r_act = in ? av : 0.f;
            r_s0 = live ? ad : 0.f;
            r_s1 = live && a.kind == 0 ? lp : 0.f;
        } else {
            const float rt = a.ret[src], vo = (a.value_clip ? a.v_old : a.ret)[src];
            r_s0 = live ? rt : 0.f;
            r_s1 = live && a.value_clip ? vo : 0.f;
        }
    };
    prefetch(blockIdx.x);   // (n_blocks <= n_tiles: every workgroup has a first tile)

    // ---- weights into LDS once (zero pads: W1 columns >= D, W3 rows past the head's width); tiles' constant zeros ----
    tsm_stage_padded<kThreadsU>(lds + ly.W1, P, kHid * ld1, ld1, kHid, D, D);
    tsm_stage_padded<kThreadsU>(lds + ly.W2, P + oW2, kHid * kLdh, kLdh, kHid, kHid, kHid);
    tsm_stage_padded<kThreadsU>(lds + ly.W3, P + oW3, kRows * kLdh, kLdh, ow, kHid, kHid);
    if (tid < kHid) { lds[ly.B1 + tid] = P[oB1 + tid]; lds[ly.B2 + tid] = P[oB2 + tid]; }
    if (tid < kMaxOut) {
        lds[ly.B3 + tid] = tid < ow ? P[oB3 + tid] : 0.f;
        lds[ly.SG + tid] = (NET == 0 && !a.cond && tid < Ad) ? P[oB3 + ow + tid] : 0.f;
    }
    for (int i = tid; i < kRows * ld1; i += kThreadsU) lds[ly.X + i] = 0.f;
    for (int i = tid; i < kRows * kLdo; i += kThreadsU) { lds[ly.OUT + i] = 0.f; lds[ly.D3 + i] = 0.f; }
    if (NET == 0 && tid == 0) {
        GuHeadC h;
        h.eps_clip = a.eps_clip; h.dual_clip = a.dual_clip; h.ent_coef = a.ent_coef; h.invM = 1.0 / (double)M;
        h.mean = 0.0; h.istd = 1.0;
        if (a.adv_norm) {   // (ppo.py:185: (adv - mean) / (std + self._eps), the statistics being tsm_ppo_adv_stats' f32 pair)
            h.mean = (double)a.adv_stats[0];
            h.istd = 1.0 / ((double)a.adv_stats[1] + 1e-8);
        }
        h.max_action = a.max_action; h.kind = a.kind; h.flags = (a.cond ? 1 : 0) | (a.unbounded ? 2 : 0) | (Ad << 8);
        *reinterpret_cast<GuHeadC *>(hc_d) = h;
    }

    const int col = 16 * w + c16;   // this lane's hidden column in the forward and input-gradient chains
    const f4 zero = {0.f, 0.f, 0.f, 0.f};
    f4 g_W3 = zero;          // rows: output kq * 4 + q; column: hidden 16 w + c16
    f4 g_W2[4], g_W1[NJ];    // rows: hidden 16 w + kq * 4 + q; columns: 16 jb + c16
#pragma unroll
    for (int j = 0; j < 4; ++j) g_W2[j] = zero;
#pragma unroll
    for (int j = 0; j < NJ; ++j) g_W1[j] = zero;
    float g_b1 = 0.f, g_b2 = 0.f, g_b3 = 0.f;   // threads < 64, < 64, < 16
    double acc_col = 0.0;                        // threads 64 + k, k < act_dim: d loss / d sigma_param[k]
    double s_a = 0.0, s_b = 0.0;                 // thread 128: actor (objective, entropy) | critic (value loss, -)

    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int64_t row0 = t * kRows;
        __syncthreads();   // (the previous tile's layer-1 gradients read X; the first tile: the staging above)
        // 0. the tile into X (columns >= D and rows past M stay / become zero)
#pragma unroll
        for (int it = 0; it < NJ; ++it) {
            const int e = tid + it * kThreadsU, r = e / D, c = e - r * D;
            if (e < kRows * D) lds[ly.X + r * ld1 + c] = xr[it];
        }
        const float c_act = r_act, c_s0 = r_s0, c_s1 = r_s1;
        __syncthreads();
        // 1. layer 1
        {
            const f4 acc = gu_chain<K1>(lds + ly.X + c16 * ld1 + kq, 1, lds + ly.W1 + col * ld1 + kq, 1, zero);
            const float b = lds[ly.B1 + col];
#pragma unroll
            for (int q = 0; q < 4; ++q) lds[ly.H1 + (kq * 4 + q) * kLdh + col] = act_fwd(acc[q] + b, act_fn);
        }
        __syncthreads();
        // 2. layer 2
        {
            const f4 acc = gu_chain<kHid>(lds + ly.H1 + c16 * kLdh + kq, 1, lds + ly.W2 + col * kLdh + kq, 1, zero);
            const float b = lds[ly.B2 + col];
#pragma unroll
            for (int q = 0; q < 4; ++q) lds[ly.H2 + (kq * 4 + q) * kLdh + col] = act_fwd(acc[q] + b, act_fn);
        }
        __syncthreads();
        // 3. output layer (linear): the raw outputs, or V in column 0
        if (w == 0) {
            const f4 acc = gu_chain<kHid>(lds + ly.H2 + c16 * kLdh + kq, 1, lds + ly.W3 + c16 * kLdh + kq, 1, zero);
            const float b = lds[ly.B3 + c16];
#pragma unroll
            for (int q = 0; q < 4; ++q) lds[ly.OUT + (kq * 4 + q) * kLdo + c16] = acc[q] + b;
        }
        __syncthreads();
        // 4. head: lane (row r, component k)
        {
            const int r = tid >> 4, k = tid & 15;
            const bool live = row0 + r < M;
            if (NET == 0) {
                gu_actor_head(reinterpret_cast<const GuHeadC *>(hc_d), lds + ly.OUT + r * kLdo, lds + ly.SG, c_act, c_s0, c_s1, k, live,
                              lds + ly.D3 + r * kLdo, s_col + r * kMaxOut + k, s_obj + r, s_ent + r);
            } else if (k == 0) {   // the value term of one sample (ppo_loss.hip's value_terms, loss_kind 2)
                const float v = lds[ly.OUT + r * kLdo], ret = c_s0;
                float vf, g_v;
                if (a.value_clip) {
                    const float vs = c_s1, eps = a.eps_clip_f;
                    const float d = v - vs;
                    const float dc = fminf(fmaxf(d, -eps), eps);
                    const bool v_in = d >= -eps && d <= eps;
                    const float vclip = vs + dc;
                    const float vf1 = (ret - v) * (ret - v), vf2 = (ret - vclip) * (ret - vclip);
                    const float g1 = 2.f * (v - ret), g2 = v_in ? 2.f * (vclip - ret) : 0.f;
                    if (vf1 > vf2) { vf = vf1; g_v = g1; }
                    else if (vf1 < vf2) { vf = vf2; g_v = g2; }
                    else { vf = vf1; g_v = 0.5f * g1 + 0.5f * g2; }
                } else {
                    vf = (ret - v) * (ret - v);
                    g_v = 2.f * (v - ret);
                }
                const float dv = a.vf_coef_f * g_v * (1.0f / (float)M);
                lds[ly.D3 + r * kLdo] = live ? dv : 0.f;
                s_obj[r] = live ? (double)vf : 0.0;
            }
        }
        __syncthreads();
        if (t + gridDim.x < n_tiles) prefetch(t + gridDim.x);   // the next tile's gathers fly under this tile's backward
        // 5. output layer: dW3 += D3^T H2, dH2 = D3 W3 through the activation's derivative, db3; the tile's f64 folds
        {
            g_W3 = gu_chain<kRows>(lds + ly.D3 + kq * kLdo + c16, kLdo, lds + ly.H2 + kq * kLdh + col, kLdh, g_W3);
            const f4 acc = gu_chain<kMaxOut>(lds + ly.D3 + c16 * kLdo + kq, 1, lds + ly.W3 + kq * kLdh + col, kLdh, zero);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int row = kq * 4 + q;
                lds[ly.D2 + row * kLdh + col] = gu_act_grad(acc[q], lds[ly.H2 + row * kLdh + col], act_fn);
            }
            if (tid < kMaxOut) g_b3 += gu_column_sum(lds + ly.D3 + tid, kLdo);
            if (NET == 0 && !a.cond && tid >= 64 && tid < 64 + Ad) {
                for (int r = 0; r < kRows; ++r) acc_col += s_col[r * kMaxOut + tid - 64];
            }
            if (tid == 128) {
                for (int r = 0; r < kRows; ++r) {
                    s_a += s_obj[r];
                    if (NET == 0) s_b += s_ent[r];
                }
            }
        }
        __syncthreads();
        // 6. layer 2: dW2 += D2^T H1, db2, dH1 = D2 W2 through the activation's derivative
        {
            const float *dA = lds + ly.D2 + kq * kLdh + col;
#pragma unroll
            for (int jb = 0; jb < 4; ++jb) g_W2[jb] = gu_chain<kRows>(dA, kLdh, lds + ly.H1 + kq * kLdh + 16 * jb + c16, kLdh, g_W2[jb]);
            if (tid < kHid) g_b2 += gu_column_sum(lds + ly.D2 + tid, kLdh);
            const f4 acc = gu_chain<kHid>(lds + ly.D2 + c16 * kLdh + kq, 1, lds + ly.W2 + kq * kLdh + col, kLdh, zero);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int row = kq * 4 + q;
                lds[ly.D1 + row * kLdh + col] = gu_act_grad(acc[q], lds[ly.H1 + row * kLdh + col], act_fn);
            }
        }
        __syncthreads();
        // 7. layer 1: dW1 += D1^T X, db1
        {
            const float *dA = lds + ly.D1 + kq * kLdh + col;
#pragma unroll
            for (int jb = 0; jb < NJ; ++jb) g_W1[jb] = gu_chain<kRows>(dA, kLdh, lds + ly.X + kq * ld1 + 16 * jb + c16, ld1, g_W1[jb]);
            if (tid < kHid) g_b1 += gu_column_sum(lds + ly.D1 + tid, kLdh);
        }
    }

    // ---- this net's columns of the workgroup's slab (consumed once, by the optimizer launch: non-temporal stores) ----
    float *S = a.slabs + (int64_t)blockIdx.x * a.slab_stride + (NET ? n_actor : 0);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int hrow = 16 * w + kq * 4 + q;
#pragma unroll
        for (int jb = 0; jb < NJ; ++jb) {
            const int c = 16 * jb + c16;
            if (c < D) __builtin_nontemporal_store(g_W1[jb][q], &S[hrow * D + c]);
        }
#pragma unroll
        for (int jb = 0; jb < 4; ++jb) __builtin_nontemporal_store(g_W2[jb][q], &S[oW2 + hrow * kHid + 16 * jb + c16]);
        if (kq * 4 + q < ow) __builtin_nontemporal_store(g_W3[q], &S[oW3 + (kq * 4 + q) * kHid + col]);
    }
    if (tid < kHid) {
        __builtin_nontemporal_store(g_b1, &S[oB1 + tid]);
        __builtin_nontemporal_store(g_b2, &S[oB2 + tid]);
    }
    if (tid < ow) __builtin_nontemporal_store(g_b3, &S[oB3 + tid]);
    if (NET == 0 && !a.cond && tid >= 64 && tid < 64 + Ad) __builtin_nontemporal_store((float)acc_col, &S[oB3 + ow + tid - 64]);
    // loss partials: actor row b = {objective, 0, entropy, 0}; critic row n_blocks + b = {0, value loss, 0, 0}
    if (tid == 128) {
        double *p = a.partial + 4 * ((int64_t)NET * gridDim.x + blockIdx.x);
        p[0] = NET ? 0.0 : s_a;
        p[1] = NET ? s_a : 0.0;
        p[2] = NET ? 0.0 : s_b;
        p[3] = 0.0;
    }
}

template <int NJ>
__global__ __launch_bounds__(kThreadsU) void ppo_update_gauss_kernel(GuArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    // device-resident optimizer step count (graph replay): bumped here, read by the Adam launch that follows
    if (a.opt_step && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *a.opt_step += 1;
    if (blockIdx.y == 0) gu_net<NJ, 0>(lds, a);
    else gu_net<NJ, 1>(lds, a);
}

template <int NJ>
int gu_launch(const GuArgs &a, int32_t n_blocks, void *stream) {
    const GuLay ly(NJ);
    const size_t shmem = (size_t)ly.total * sizeof(float);
    static bool attr_set = false;
    if (!attr_set) {
        TSM_HIP(tsm_allow_max_lds(reinterpret_cast<const void *>(ppo_update_gauss_kernel<NJ>)));
        attr_set = true;
    }
    hipLaunchKernelGGL(ppo_update_gauss_kernel<NJ>, dim3((unsigned)n_blocks, 2), dim3(kThreadsU), shmem, tsm_stream(stream), a);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

int gu_check(const char *who, int32_t obs_dim, int32_t hidden, int32_t act_dim, int32_t conditioned_sigma, int32_t act_kind) {
    TSM_REQUIRE(hidden == kHid, "%s: both hidden layers must be %d wide (got %d)", who, kHid, hidden);
    TSM_REQUIRE(obs_dim >= 1 && obs_dim <= 16 * kMaxNJ, "%s: obs_dim = %d outside [1, %d]", who, obs_dim, 16 * kMaxNJ);
    const int64_t ow = (int64_t)act_dim * (conditioned_sigma ? 2 : 1);
    TSM_REQUIRE(act_dim >= 1 && ow <= kMaxOut, "%s: actor output width %sact_dim = %lld outside [1, %d]", who,
                conditioned_sigma ? "2 * " : "", (long long)ow, kMaxOut);
    TSM_REQUIRE(act_kind == 1 || act_kind == 2, "%s: activation must be 1 (relu) or 2 (tanh), got %d", who, act_kind);
    return TSM_OK;
}

}  // namespace

TSM_EXPORT int tsm_ppo_update_gauss_check(int32_t obs_dim, int32_t hidden, int32_t act_dim, int32_t conditioned_sigma,
                                          int32_t act_kind) {
    return gu_check("tsm_ppo_update_gauss_check", obs_dim, hidden, act_dim, conditioned_sigma, act_kind);
}

TSM_EXPORT int tsm_ppo_update_gauss_grid(int64_t M, int32_t *n_blocks_out) {
    // tsm_ppo_update_grid's rule (csrc/mlp_fused.hip), whose sweeps were taken on this work split: a slab of the two 64-64 nets is
    // 45 KB written here and read back by Adam, and two workgroups of <= 64.4 KB LDS fit a CU, so one tile per workgroup pair up to
    // 256 tiles, two up to 512, then 256 / 384 pairs walking their tiles.
    TSM_REQUIRE(n_blocks_out, "tsm_ppo_update_gauss_grid: null pointer");
    TSM_REQUIRE(M >= 1, "tsm_ppo_update_gauss_grid: M must be >= 1");
    const int64_t n_tiles = ceil_div(M, kRows);
    int64_t g;
    if (n_tiles <= 256) g = n_tiles;
    else if (n_tiles < 1024) g = (n_tiles + 1) / 2 < 256 ? (n_tiles + 1) / 2 : 256;
    else g = 384;
    *n_blocks_out = (int32_t)g;
    return TSM_OK;
}

TSM_EXPORT int tsm_ppo_update_gauss(const float *params, int32_t obs_dim, int32_t hidden, int32_t act_dim, int32_t conditioned_sigma,
                                    int32_t act_kind, double max_action, int32_t unbounded, const float *obs, const float *act,
                                    const float *logp_old, const float *adv, const float *returns, const float *v_s_old,
                                    const int64_t *perm, int64_t first_row, int64_t M, const float *adv_stats,
                                    const tsm_ppo_cfg *cfg_host, int32_t n_blocks, float *grad_slabs_out, int64_t slab_stride,
                                    double *loss_partial_out, int64_t *opt_step_dev, void *stream) {
    if (int rc = gu_check("tsm_ppo_update_gauss", obs_dim, hidden, act_dim, conditioned_sigma, act_kind)) return rc;
    TSM_REQUIRE(M >= 1 && M <= (int64_t)1 << 40, "tsm_ppo_update_gauss: M = %lld out of range", (long long)M);
    TSM_REQUIRE(cfg_host, "tsm_ppo_update_gauss: null cfg");
    TSM_REQUIRE(cfg_host->loss_kind == 0 || cfg_host->loss_kind == 1, "tsm_ppo_update_gauss: loss_kind must be 0 or 1");
    TSM_REQUIRE(params && obs && act && adv && returns && grad_slabs_out && loss_partial_out && (cfg_host->loss_kind == 1 || logp_old),
                "tsm_ppo_update_gauss: null pointer");
    TSM_REQUIRE(!cfg_host->value_clip || v_s_old, "tsm_ppo_update_gauss: value_clip needs v_s_old");
    TSM_REQUIRE(!cfg_host->adv_norm || adv_stats, "tsm_ppo_update_gauss: adv_norm needs adv_stats");
    TSM_REQUIRE(cfg_host->dual_clip <= 0.0 || cfg_host->dual_clip > 1.0,
                "Dual-clip PPO parameter should greater than 1.0 but got %g", cfg_host->dual_clip);  // ppo.py:124-126
    TSM_REQUIRE(first_row >= 0, "tsm_ppo_update_gauss: negative first_row");
    TSM_REQUIRE(n_blocks >= 1 && n_blocks <= ceil_div(M, kRows), "tsm_ppo_update_gauss: n_blocks = %d outside [1, ceil(M / 16) = %lld]",
                n_blocks, (long long)ceil_div(M, kRows));
    const int ow = act_dim * (conditioned_sigma ? 2 : 1);
    const int64_t n_param = 2 * ((int64_t)kHid * obs_dim + 2 * kHid + kHid * kHid) + (ow + 1) * (kHid + 1) + (conditioned_sigma ? 0 : act_dim);
    TSM_REQUIRE(slab_stride >= n_param, "tsm_ppo_update_gauss: slab_stride %lld smaller than the parameter count %lld",
                (long long)slab_stride, (long long)n_param);
    GuArgs a{};
    a.P = params; a.D = obs_dim; a.Ad = act_dim; a.out_w = ow; a.cond = conditioned_sigma != 0; a.act_fn = act_kind;
    a.unbounded = unbounded != 0; a.max_action = (double)(float)max_action;   // (f32, as tsm_gauss_ppo_head takes it)
    a.obs = obs; a.act = act; a.logp_old = logp_old; a.adv = adv; a.ret = returns; a.v_old = v_s_old;
    a.perm = perm; a.first = first_row; a.M = M; a.adv_stats = adv_stats;
    a.eps_clip = cfg_host->eps_clip; a.dual_clip = cfg_host->dual_clip; a.ent_coef = cfg_host->ent_coef;
    a.eps_clip_f = (float)cfg_host->eps_clip; a.vf_coef_f = (float)cfg_host->vf_coef;
    a.value_clip = cfg_host->value_clip; a.adv_norm = cfg_host->adv_norm; a.kind = cfg_host->loss_kind;
    a.slabs = grad_slabs_out; a.slab_stride = slab_stride; a.partial = loss_partial_out; a.opt_step = opt_step_dev;
    const int nJ = (obs_dim + 15) / 16;
    return nJ == 1 ? gu_launch<1>(a, n_blocks, stream) : nJ == 2 ? gu_launch<2>(a, n_blocks, stream)
           : nJ == 3 ? gu_launch<3>(a, n_blocks, stream) : gu_launch<4>(a, n_blocks, stream);
}
