// rollout_gauss.hip -- persistent rollout for Box actions: the whole Collector loop of one collect(n_step) call of a Gaussian
// GenericPPO on continuous simple_spread in ONE launch.
//
// Fuses, per vector step and without leaving the chip, what the per-step device loop runs as about ten launches:
//   actor forward (and the critic's, when it sees the agent's own observation)        tsm_mlp_forward (csrc/dense.hip)
//   Independent(Normal(mu, sigma), 1): sample or mode, log-probability, map_action    tsm_gauss_sample (csrc/gauss.hip)
//   the Box env step with resets of finished envs                                     tsm_mpe_spread_step_box (csrc/mpe.hip)
//   buffer.add: index algebra + payload scatter (act f32 [5])                         tsm_vrb_add (csrc/vrb.hip)
// Every result is bit-identical to that sequence (tests/test_gpu_rollout_gauss.py): the layers are v_mfma_f32_16x16x4_f32 chains in
// dense.hip's k order (ascending k-steps of 4 over the zero-padded multiple of 16, one chain per output element, bias after the
// chain, gemm_tile_dev.h's activation), the head is gauss_dev.h's arithmetic in f64 on groups of 8 lanes, the env step is
// mpe_dev.h's, the bookkeeping vrb_dev.h's / rollout_dev.h's.
//
// Work split.  A workgroup of eight waves owns EPB = 16 / N whole envs (<= 16 agent rows = one MFMA row tile) for all T steps.
// Both 64-wide nets are staged in LDS once, env state lives in LDS, only buffer rows travel to HBM.  The critic is a template flag:
// with a centralized critic (CRITIC = false) its weights are not staged, its chains not run and vs_store not written.
//
// LDS (floats; ld1 = 16 NJ + 2, ldh = 66: the pads of the [lane & 15][lane >> 4] operand reads; 95 KB at D = 48 with the critic):
//   W1a W1c [64][ld1] | W2a W2c [64][ldh] | W3a W3c [16][ldh] (rows past the head's width zero) | B1 B2 [2][64] | B3a B3c [16]
//   SG [8] sigma_param | LO HI [8] map_action's bounds | X0 X1 [16][ld1] the observation tiles, swapped every step (obs_next of
//   step t is obs of step t + 1) | H1a H1c H2a H2c [16][ldh] | RAW [16][16] the actor's raw outputs | VAL [16] | Z [2][80] the
//   normals of step t (generation t & 1) | ACT EACT [16][5] the raw sample and its map_action | AP AV LP [16][2] | REW LOGP MIN
//   [16] | STEPS DONE [16] | ROW EP [16] 64-bit | CX CY CV [16][8] pair forces | ANY
//
// Per-step phases (a barrier behind each):
//   1. layer 1: waves 0-3 one 16-column block of the actor each, waves 4-7 of the critic
//   2. layer 2: the same split
//   3. layer 3 on waves 0 (actor: 5 or 10 outputs in one 16-column block) and 4 (critic: column 0); beside it wave 7's env lanes
//      run the step's buffer index algebra (VrbLane::add) and leave row slots, done flags and "an episode ends" in LDS
//   4. head on waves 0-1: 16 rows x 8 lanes, gauss_lane -> sample -> gauss_row -> gauss_env_action; beside it waves 2-3 evaluate
//      the 16 x 8 pair forces of the env step (they depend on positions only) and waves 5-6 draw step t + 1's normals
//   5. move: one lane per agent folds its pair forces in partner order onto mpe_box_action_force, integrates, publishes
//   6. reward terms (landmark minima, collisions) on the agent lanes; the other waves build the obs_next tile
//   7. rewards; then, with no barrier between, 8. the scatter: obs / obs_next elements over all threads, the rows' payload on wave
//      1, the episode returns on the env lanes
//   9. only where an episode ended: episode counters, re-initialised envs, their first observation into the next tile
#include "common.h"
#include "gauss_dev.h"
#include "gemm_tile_dev.h"
#include "mpe_dev.h"
#include "philox.h"
#include "rollout_dev.h"

int tsm_mpe_check_cfg(const tsm_mpe_cfg *h, MpeCfg *c);  // mpe.hip

namespace {

constexpr int kRows = 16, kHid = 64, kLdh = kHid + 2, kThreadsG = 512, kAd = kMpeBoxDim, kZ = kRows * kAd;

struct GrLay {   // offsets in floats
    int ld1, W1a, W1c, W2a, W2c, W3a, W3c, B1, B2, B3a, B3c, SG, LO, HI, X0, X1, H1a, H1c, H2a, H2c, RAW, VAL, Z, ACT, EACT, AP, AV,
        LP, REW, LOGP, MIN, STEPS, DONE, ROW, EP, CX, CY, CV, ANY, total;
    __host__ __device__ GrLay(int NJ, bool critic) {
        ld1 = 16 * NJ + 2;
        int o = 0;
        W1a = o; o += kHid * ld1;
        W1c = o; o += critic ? kHid * ld1 : 0;
        W2a = o; o += kHid * kLdh;
        W2c = o; o += critic ? kHid * kLdh : 0;
        W3a = o; o += kRows * kLdh;
        W3c = o; o += critic ? kRows * kLdh : 0;
        B1 = o; o += 2 * kHid;      // actor | critic
        B2 = o; o += 2 * kHid;
        B3a = o; o += 16;
        B3c = o; o += 16;
        SG = o; o += 8;
        LO = o; o += 8;
        HI = o; o += 8;
        X0 = o; o += kRows * ld1;
        X1 = o; o += kRows * ld1;
        H1a = o; o += kRows * kLdh;
        H1c = o; o += critic ? kRows * kLdh : 0;
        H2a = o; o += kRows * kLdh;
        H2c = o; o += critic ? kRows * kLdh : 0;
        RAW = o; o += kRows * 16;
        VAL = o; o += kRows;
        Z = o; o += 2 * kZ;
        ACT = o; o += kZ;
        EACT = o; o += kZ;
        AP = o; o += kRows * 2;
        AV = o; o += kRows * 2;
        LP = o; o += kRows * 2;
        REW = o; o += kRows;
        LOGP = o; o += kRows;
        MIN = o; o += kRows;
        STEPS = o; o += kRows;      // int [EPB]
        DONE = o; o += kRows;       // int [EPB]
        o = (o + 1) & ~1;           // (8-byte alignment by index arithmetic off the 16-byte aligned base)
        ROW = o; o += 2 * kRows;    // int64 [EPB]
        EP = o; o += 2 * kRows;     // uint64 [EPB]
        o = (o + 3) & ~3;
        CX = o; o += kRows * 8;     // [16][8], 16-byte rows (mpe_pair_fold)
        CY = o; o += kRows * 8;
        CV = o; o += kRows * 8;     // int
        ANY = o; o += 4;            // int
        total = o;
    }
};

struct GrArgs {
    const float *P;            // actor w0 b0 w1 b1 w2 b2 [sigma_param] | critic w0 b0 w1 b1 w2 b2
    int D, out_w, act_fn;      // out_w: 5, or 10 with a conditioned sigma; act_fn: 1 relu, 2 tanh
    int cond, unbounded, bound, deterministic;
    float max_action;
    const float *low, *high;   // nullable together
    uint64_t pol_seed, offset;
    const uint64_t *offset_dev;
    MpeCfg c;
    uint64_t env_seed;
    uint64_t *episode_ctr;
    float *apos, *avel, *lpos;
    int32_t *steps;
    int auto_reset;
    float *obs_cur_out;
    float *act_f32;            // [S][B][N][5]
    RolloutBufArgs b;          // (b.act_store, b.vnext_store: unused here)
};

__device__ __forceinline__ f4 gr_mfma4(float a, float b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// One 16 x 16 output block of a layer: rows = the tile's 16 samples, columns = the 16 outputs whose weight rows start at `w`
// (this lane's: w + c16 * ldw + kq).  dense.hip's chain: acc <- mfma(x[k0 .. k0 + 4), w[k0 .. k0 + 4), acc), k0 ascending.
template <int K>
__device__ __forceinline__ f4 gr_block(const float *x, const float *w) {
    f4 acc = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k0 = 0; k0 < K; k0 += 4) acc = gr_mfma4(x[k0], w[k0], acc);
    return acc;
}

// The head of one row on a group of 8 lanes (kept out of line: the f64 tanh / exp of device libm would otherwise sit in the
// register budget of the whole step loop).
__device__ __noinline__ void gr_head(const float *raw, const float *sg_row, const float *s_lo, const float *s_hi, bool cond,
                                     bool unbounded, int bound, float max_action, float zf, bool in, bool live, int k, float *act,
                                     float *eact, float *logp_out) {
    GaussLane o;
    gauss_lane(raw, sg_row, cond, in, k, (double)max_action, unbounded, o);
    const double zn = in ? (double)zf : 0.0;
    const float a = (float)(o.mu + o.sigma * zn);   // the mode draws nothing (zf = 0): mu
    double z;
    const double logp = gauss_row<8>(o, a, in, z);
    if (in && live) {
        act[k] = a;
        eact[k] = gauss_env_action(a, bound, s_lo, s_hi, k);
    }
    if (k == 0 && live) *logp_out = (float)logp;
}

template <int NJ, bool CRITIC>
__global__ __launch_bounds__(kThreadsG) void rollout_gauss_kernel(GrArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const MpeCfg c = a.c;
    const GrLay ly(NJ, CRITIC);
    constexpr int ld1 = 16 * NJ + 2, K1 = 16 * NJ;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c16 = lane & 15, kq = lane >> 4;
    const int N = c.N, D = a.D, st = 2 * N;
    const int EPB = kRows / N;
    const int e0 = blockIdx.x * EPB;
    const int n_here = min(EPB, c.n_env - e0);
    const int rows_here = n_here * N;         // live tile rows: row r = (env el, agent ai), r = el * N + ai
    const int64_t B = c.n_env;
    float *s_ap = lds + ly.AP, *s_av = lds + ly.AV, *s_lp = lds + ly.LP, *s_rew = lds + ly.REW, *s_logp = lds + ly.LOGP,
          *s_m = lds + ly.MIN, *s_cx = lds + ly.CX, *s_cy = lds + ly.CY, *s_act = lds + ly.ACT, *s_eact = lds + ly.EACT,
          *s_z = lds + ly.Z, *s_val = lds + ly.VAL;
    int *s_steps = reinterpret_cast<int *>(lds + ly.STEPS), *s_done = reinterpret_cast<int *>(lds + ly.DONE),
        *s_cv = reinterpret_cast<int *>(lds + ly.CV), *s_any = reinterpret_cast<int *>(lds + ly.ANY);
    int64_t *s_row = reinterpret_cast<int64_t *>(lds + ly.ROW);
    uint64_t *s_ep = reinterpret_cast<uint64_t *>(lds + ly.EP);

    // ---- weights into LDS once (zero pads: W1 columns >= D, W3 rows past the head's width) ----
    {
        const int ow = a.out_w;
        const int oB1 = kHid * D, oW2 = oB1 + kHid, oB2 = oW2 + kHid * kHid, oW3 = oB2 + kHid, oB3 = oW3 + ow * kHid;
        const int n_actor = oB3 + ow + (a.cond ? 0 : kAd);
        tsm_stage_padded<kThreadsG>(lds + ly.W1a, a.P, kHid * ld1, ld1, kHid, D, D);
        tsm_stage_padded<kThreadsG>(lds + ly.W2a, a.P + oW2, kHid * kLdh, kLdh, kHid, kHid, kHid);
        tsm_stage_padded<kThreadsG>(lds + ly.W3a, a.P + oW3, kRows * kLdh, kLdh, ow, kHid, kHid);
        if (tid < kHid) { lds[ly.B1 + tid] = a.P[oB1 + tid]; lds[ly.B2 + tid] = a.P[oB2 + tid]; }
        if (tid < 16) lds[ly.B3a + tid] = tid < ow ? a.P[oB3 + tid] : 0.f;
        if (tid < 8) {
            lds[ly.SG + tid] = (!a.cond && tid < kAd) ? a.P[oB3 + ow + tid] : 0.f;
            lds[ly.LO + tid] = (a.low && tid < kAd) ? a.low[tid] : 0.f;
            lds[ly.HI + tid] = (a.low && tid < kAd) ? a.high[tid] : 0.f;
        }
        if constexpr (CRITIC) {
            const float *Pc = a.P + n_actor;
            const int cB3 = oW3 + kHid;   // the critic's last layer has one row
            tsm_stage_padded<kThreadsG>(lds + ly.W1c, Pc, kHid * ld1, ld1, kHid, D, D);
            tsm_stage_padded<kThreadsG>(lds + ly.W2c, Pc + oW2, kHid * kLdh, kLdh, kHid, kHid, kHid);
            tsm_stage_padded<kThreadsG>(lds + ly.W3c, Pc + oW3, kRows * kLdh, kLdh, 1, kHid, kHid);
            if (tid < kHid) { lds[ly.B1 + kHid + tid] = Pc[oB1 + tid]; lds[ly.B2 + kHid + tid] = Pc[oB2 + tid]; }
            if (tid < 16) lds[ly.B3c + tid] = tid == 0 ? Pc[cB3] : 0.f;
        }
    }
    for (int i = tid; i < kRows * ld1; i += kThreadsG) { lds[ly.X0 + i] = 0.f; lds[ly.X1 + i] = 0.f; }

    const VrbState vs = vrb_view(a.b.vrb_state, B, N);
    // agent lane r = tid < rows_here (wave 0) <-> (env el, agent ai); env lane 448 + bel (wave 7) owns env bel's bookkeeping
    const int r = tid, el = r / N, ai = r - el * N;
    const bool lane_live = r < rows_here;
    const int e = e0 + el;
    const int bel = tid - 448;
    const bool env_lane = bel >= 0 && bel < n_here;
    const int be = e0 + bel;
    VrbLane vl;
    EpReturns<kMpeMaxN> epr;
    if (env_lane) {
        vl.load(vs, be);
        epr.load(vs, N, be);
        s_steps[bel] = a.steps[be];
        s_done[bel] = 0;
        s_row[bel] = 0;
    }
    for (int i = tid; i < n_here * st; i += kThreadsG) {
        s_ap[i] = a.apos[(int64_t)e0 * st + i];
        s_av[i] = a.avel[(int64_t)e0 * st + i];
        s_lp[i] = a.lpos[(int64_t)e0 * st + i];
    }
    const uint64_t off0 = a.offset + (a.offset_dev ? *a.offset_dev : 0ull);
    // the normals of (step, row, component): lanes zl < 80 of waves 5-6 <-> (row zl / 5, component zl % 5); element index
    // (env * N + agent) * 5 + k at the counter off0 + t * n_env * N * 5, as the per-step tsm_gauss_sample launches see them
    const int zl = tid - 320, zr = zl / kAd;
    const bool z_lane = !a.deterministic && zl >= 0 && zl < kZ && zr < rows_here;
    const int64_t z_elem = ((int64_t)e0 * N + zr) * kAd + (zl - zr * kAd);
    const uint64_t step_draws = (uint64_t)B * (uint64_t)N * (uint64_t)kAd;
    if (zl >= 0 && zl < kZ) {   // (the mode, and rows that do not exist, draw nothing: their cells stay 0)
        s_z[zl] = z_lane ? gauss_normal(a.pol_seed, off0, z_elem) : 0.f;
        s_z[kZ + zl] = 0.f;
    }
    // the pair (agent row, other agent) tasks of the env step on waves 2-3: task p = tid - 128 -> row p >> 3, other p & 7
    const int pt = tid - 128;
    int pair_ei = -1;
    if (pt >= 0 && pt < kRows * 8) {
        const int rp = pt >> 3, ep = rp / N;
        pair_ei = rp < rows_here ? (ep << 3) | (rp - ep * N) : -1;
    }
    __syncthreads();
    int xcur = ly.X0, xnxt = ly.X1;
    for (int i = tid; i < rows_here * D; i += kThreadsG) {
        const int rr = i / D, k = i - rr * D, ee = rr / N;
        lds[xcur + rr * ld1 + k] = mpe_obs_elem(c, s_ap + ee * st, s_av + ee * st, s_lp + ee * st, rr - ee * N, k);
    }
    __syncthreads();

    // this wave's chain in layers 1 and 2: net = actor (waves 0-3) or critic (4-7), column block w & 3
    const bool critic_w = w >= 4;
    const bool chain_w = CRITIC || !critic_w;
    const int col = 16 * (w & 3) + c16;
    const float *w1 = lds + (critic_w ? ly.W1c : ly.W1a) + col * ld1 + kq;
    const float *w2 = lds + (critic_w ? ly.W2c : ly.W2a) + col * kLdh + kq;
    const float *w3 = lds + (critic_w ? ly.W3c : ly.W3a) + c16 * kLdh + kq;
    float *h1 = lds + (critic_w ? ly.H1c : ly.H1a), *h2 = lds + (critic_w ? ly.H2c : ly.H2a);
    const float b1 = lds[ly.B1 + (critic_w ? kHid : 0) + col], b2 = lds[ly.B2 + (critic_w ? kHid : 0) + col];
    const float b3 = lds[(critic_w ? ly.B3c : ly.B3a) + c16];

    for (int t = 0; t < a.b.n_steps; ++t) {
        float *XN = lds + xnxt;
        // 1. layer 1
        if (chain_w) {
            const f4 acc = gr_block<K1>(lds + xcur + c16 * ld1 + kq, w1);
#pragma unroll
            for (int q = 0; q < 4; ++q) h1[(kq * 4 + q) * kLdh + col] = act_fwd(acc[q] + b1, a.act_fn);
        }
        __syncthreads();
        // 2. layer 2
        if (chain_w) {
            const f4 acc = gr_block<kHid>(h1 + c16 * kLdh + kq, w2);
#pragma unroll
            for (int q = 0; q < 4; ++q) h2[(kq * 4 + q) * kLdh + col] = act_fwd(acc[q] + b2, a.act_fn);
        }
        __syncthreads();
        // 3. layer 3 (linear): the actor's raw outputs on wave 0, the critic's value (column 0) on wave 4
        if (chain_w && (w & 3) == 0) {
            const f4 acc = gr_block<kHid>(h2 + c16 * kLdh + kq, w3);
            if (!critic_w) {
#pragma unroll
                for (int q = 0; q < 4; ++q) lds[ly.RAW + (kq * 4 + q) * 16 + c16] = acc[q] + b3;
            } else if (c16 == 0) {
#pragma unroll
                for (int q = 0; q < 4; ++q) s_val[kq * 4 + q] = acc[q] + b3;
            }
        }
        //    ... beside it the buffer index algebra of this step on the env lanes (buffer_base.py:373-410 + manager.py:170-177)
        bool tr = false, rec = false;
        int64_t o = 0;
        if (env_lane) {
            const int stp = s_steps[bel] + 1;
            tr = stp >= c.max_cycles;
            s_steps[bel] = stp;
            const VrbStep sp = vl.add(vs, a.b.S, t, be, B, tr, a.b.done_store, a.b.ptr_out, a.b.ep_len_out, a.b.ep_idx_out, a.b.ep_rec, a.b.max_ep);
            o = sp.o; rec = sp.rec;
            s_row[bel] = sp.row;
            s_done[bel] = tr ? 1 : 0;
            const unsigned long long ends = __ballot(tr);   // (the env lanes share wave 7)
            if (bel == 0) s_any[0] = ends != 0ull;
        }
        __syncthreads();
        // 4. head on waves 0-1; pair forces on waves 2-3; the next step's normals on waves 5-6
        if (tid < kRows * 8) {
            const int hr = tid >> 3, k = tid & 7;
            const bool in = k < kAd;
            const float *raw = lds + ly.RAW + hr * 16;
            gr_head(raw, a.cond ? raw + kAd : lds + ly.SG, a.low ? lds + ly.LO : nullptr, lds + ly.HI, a.cond != 0, a.unbounded != 0,
                    a.bound, a.max_action, in ? s_z[(t & 1) * kZ + hr * kAd + k] : 0.f, in, hr < rows_here, k, s_act + hr * kAd,
                    s_eact + hr * kAd, s_logp + hr);
        } else if (pt >= 0 && pt < kRows * 8) {
            const int jp = pt & 7;
            float sx = 0.f, sy = 0.f;
            int ok = 0;
            if (pair_ei >= 0 && jp < N) {
                const int ip = pair_ei & 7;
                const float *ap = s_ap + (pair_ei >> 3) * st;
                if (jp != ip) ok = mpe_pair_force(c, ap[2 * ip], ap[2 * ip + 1], ap[2 * jp], ap[2 * jp + 1], ip, jp, sx, sy) ? 1 : 0;
            }
            s_cx[pt] = sx; s_cy[pt] = sy; s_cv[pt] = ok;
        } else if (z_lane && t + 1 < a.b.n_steps) {
            s_z[((t + 1) & 1) * kZ + zl] = gauss_normal(a.pol_seed, off0 + (uint64_t)(t + 1) * step_draws, z_elem);
        }
        __syncthreads();
        // 5. env step (mpe_dev.h): the Box action force of the mapped action, the pair forces in partner order, integrate, publish
        if (lane_live) {
            const float px = s_ap[el * st + 2 * ai], py = s_ap[el * st + 2 * ai + 1];
            const float vx = s_av[el * st + 2 * ai], vy = s_av[el * st + 2 * ai + 1];
            float fx, fy;
            mpe_box_action_force(s_eact + r * kAd, c.accel, fx, fy);
            mpe_pair_fold(c, s_cx, s_cy, s_cv, r, fx, fy);
            float npx, npy, nvx, nvy;
            mpe_integrate(c, px, py, vx, vy, fx, fy, npx, npy, nvx, nvy);
            s_ap[el * st + 2 * ai] = npx; s_ap[el * st + 2 * ai + 1] = npy;
            s_av[el * st + 2 * ai] = nvx; s_av[el * st + 2 * ai + 1] = nvy;
        }
        __syncthreads();
        // 6. reward terms on wave 0; obs_next rows (the terminal observation for finished episodes) on the others
        float local = 0.f;
        if (lane_live) {
            const MpePos pos = mpe_load_pos(c, s_ap + el * st);
            s_m[r] = mpe_landmark_min_dist(c, pos, s_lp + el * st, ai);
            local = mpe_local_penalty(c, pos, s_ap + el * st, ai);
        }
        if (tid >= 64)
            for (int i = tid - 64; i < rows_here * D; i += kThreadsG - 64) {
                const int rr = i / D, k = i - rr * D, ee = rr / N;
                XN[rr * ld1 + k] = mpe_obs_elem(c, s_ap + ee * st, s_av + ee * st, s_lp + ee * st, rr - ee * N, k);
            }
        __syncthreads();
        // 7. rewards
        if (lane_live) s_rew[r] = mpe_reward(c, s_m + el * N, local);
        __syncthreads();
        // 8. payload scatter into the time-major SoA store (rows of consecutive envs are adjacent); episode returns
        if (env_lane) epr.fold(a.b.ep_rew_out, a.b.ep_rec, a.b.max_ep, N, B, be, o, tr, rec, vl.n_fin, s_rew + bel * N);
        for (int i = tid; i < rows_here * D; i += kThreadsG) {
            const int rr = i / D, k = i - rr * D, ee = rr / N;
            const int64_t dst = (s_row[ee] * N + (rr - ee * N)) * D + k;
            a.b.obs_store[dst] = lds[xcur + rr * ld1 + k];
            if (a.b.obs_next_store) a.b.obs_next_store[dst] = XN[rr * ld1 + k];
        }
        {
            const int ur = tid - 64;   // the rows' payload on wave 1
            if (ur >= 0 && ur < rows_here) {
                const int pel = ur / N, pai = ur - pel * N;
                const int64_t dst = s_row[pel] * N + pai;
#pragma unroll
                for (int k = 0; k < kAd; ++k) a.act_f32[dst * kAd + k] = s_act[ur * kAd + k];
                a.b.rew_store[dst] = s_rew[ur];
                a.b.term_store[dst] = 0;
                a.b.trunc_store[dst] = (uint8_t)s_done[pel];
                if (a.b.logp_store) a.b.logp_store[dst] = s_logp[ur];
                if (CRITIC && a.b.vs_store) a.b.vs_store[dst] = s_val[ur];
            }
        }
        // 9. finished episodes: re-initialise the env; its first observation replaces the terminal one in the next tile
        if (s_any[0] && a.auto_reset) {   // (uniform: written in phase 3)
            if (env_lane && s_done[bel]) {
                const uint64_t ep = a.episode_ctr[be];
                s_ep[bel] = ep;
                a.episode_ctr[be] = ep + 1;
                s_steps[bel] = 0;
            }
            __syncthreads();   // (also: every thread has stored its obs_next elements)
            if (lane_live && s_done[el])
                mpe_reset_agent(c, e, a.env_seed, s_ep[el], ai, s_ap + el * st, s_av + el * st, s_lp + el * st);
            __syncthreads();
            for (int i = tid; i < rows_here * D; i += kThreadsG) {
                const int rr = i / D, k = i - rr * D, ee = rr / N;
                if (s_done[ee]) XN[rr * ld1 + k] = mpe_obs_elem(c, s_ap + ee * st, s_av + ee * st, s_lp + ee * st, rr - ee * N, k);
            }
        }
        __syncthreads();   // the next layer 1 reads the tile; the next phase 3 rewrites the row slots this scatter read
        { const int tmp = xcur; xcur = xnxt; xnxt = tmp; }
    }
    // the observation of the next collect() call, env state and sub-buffer bookkeeping back to HBM
    if (a.obs_cur_out)
        for (int i = tid; i < rows_here * D; i += kThreadsG) {
            const int rr = i / D, k = i - rr * D;
            a.obs_cur_out[((int64_t)e0 * N + rr) * D + k] = lds[xcur + rr * ld1 + k];
        }
    for (int i = tid; i < n_here * st; i += kThreadsG) {
        a.apos[(int64_t)e0 * st + i] = s_ap[i];
        a.avel[(int64_t)e0 * st + i] = s_av[i];
        a.lpos[(int64_t)e0 * st + i] = s_lp[i];
    }
    if (env_lane) {
        a.steps[be] = s_steps[bel];
        vl.store(vs, a.b.ep_rec, be);
        epr.store(vs, N, be);
    }
    rollout_advance_counter(a.b.done_ctr, a.b.offset_dev_rw, a.b.offset_inc, tid == 0);   // (every workgroup read it before its loop)
}

template <int NJ, bool CRITIC>
int gr_launch(const GrArgs &a, void *stream) {
    const GrLay ly(NJ, CRITIC);
    const size_t shmem = (size_t)ly.total * sizeof(float);
    TSM_REQUIRE(shmem <= kTsmMaxLds, "tsm_rollout_spread_gauss: LDS layout of %zu bytes does not fit", shmem);
    static bool attr_set = false;
    if (!attr_set) {
        TSM_HIP(tsm_allow_max_lds(reinterpret_cast<const void *>(rollout_gauss_kernel<NJ, CRITIC>)));
        attr_set = true;
    }
    const unsigned n_wg = (unsigned)ceil_div(a.c.n_env, kRows / a.c.N);
    hipLaunchKernelGGL((rollout_gauss_kernel<NJ, CRITIC>), dim3(n_wg), dim3(kThreadsG), shmem, tsm_stream(stream), a);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

}  // namespace

TSM_EXPORT int tsm_rollout_spread_gauss(const tsm_rollout_desc *desc_host, float *act_store, int32_t act_dim,
                                        int32_t conditioned_sigma, int32_t unbounded, double max_action, int32_t bound_method,
                                        const float *low, const float *high, int32_t activation, int32_t run_critic, void *stream) {
    TSM_REQUIRE(desc_host, "tsm_rollout_spread_gauss: null descriptor");
    tsm_rollout_desc h = *desc_host;
    GrArgs a{};
    if (int rc = tsm_mpe_check_cfg(&h.env, &a.c)) return rc;
    TSM_REQUIRE(h.hidden == kHid, "tsm_rollout_spread_gauss: hidden must be 64 (got %d)", h.hidden);
    TSM_REQUIRE(a.c.obs_dim == h.obs_dim && h.obs_dim <= 48, "tsm_rollout_spread_gauss: obs_dim %d != 6 * n_agent (<= 48)", h.obs_dim);
    TSM_REQUIRE(h.n_act == kAd && act_dim == kAd, "tsm_rollout_spread_gauss: continuous simple_spread has Box(5,) actions");
    TSM_REQUIRE(h.n_steps >= 1 && h.sub_size >= 1, "tsm_rollout_spread_gauss: bad n_steps / sub_size");
    TSM_REQUIRE(h.mode == 1 || h.mode == 2, "tsm_rollout_spread_gauss: mode must be 1 (sample) or 2 (the mode)");
    TSM_REQUIRE(activation == 1 || activation == 2, "tsm_rollout_spread_gauss: activation must be 1 (relu) or 2 (tanh)");
    TSM_REQUIRE(bound_method >= 0 && bound_method <= 2, "tsm_rollout_spread_gauss: bound_method must be 0 (none), 1 (clip) or 2 (tanh)");
    TSM_REQUIRE((low == nullptr) == (high == nullptr), "tsm_rollout_spread_gauss: low and high come together");
    TSM_REQUIRE(h.params && act_store && h.episode_ctr && h.agent_pos && h.agent_vel && h.landmark_pos && h.steps,
                "tsm_rollout_spread_gauss: null pointer");
    h.act_store = reinterpret_cast<int32_t *>(act_store);   // (the shared check asks for an action store: this rollout's is f32)
    if (int rc = rollout_buf_args(h, "tsm_rollout_spread_gauss", &a.b)) return rc;
    a.b.vnext_store = nullptr;
    if (!run_critic) a.b.vs_store = nullptr;
    a.P = h.params; a.D = h.obs_dim; a.out_w = conditioned_sigma ? 2 * kAd : kAd; a.act_fn = activation;
    a.cond = conditioned_sigma != 0; a.unbounded = unbounded != 0; a.bound = bound_method; a.deterministic = h.mode == 2;
    a.max_action = (float)max_action; a.low = low; a.high = high;
    a.pol_seed = h.policy_seed; a.offset = h.offset; a.offset_dev = h.offset_dev;
    a.env_seed = h.env_seed; a.episode_ctr = h.episode_ctr;
    a.apos = h.agent_pos; a.avel = h.agent_vel; a.lpos = h.landmark_pos; a.steps = h.steps;
    a.auto_reset = h.auto_reset; a.obs_cur_out = h.obs_cur_out; a.act_f32 = act_store;
    const int nJ = (h.obs_dim + 15) / 16;
    if (run_critic) return nJ == 1 ? gr_launch<1, true>(a, stream) : nJ == 2 ? gr_launch<2, true>(a, stream) : gr_launch<3, true>(a, stream);
    return nJ == 1 ? gr_launch<1, false>(a, stream) : nJ == 2 ? gr_launch<2, false>(a, stream) : gr_launch<3, false>(a, stream);
}
