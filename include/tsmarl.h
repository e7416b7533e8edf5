/*
 * tsmarl.h -- C-ABI of the MI355X-native multi-agent rollout + update hot path.
 *
 * Drop-in boundary for the data-parallel hot path of eric-downes/tianshou_marl
 * (BASELINE.json north_star; scope table SURVEY.md section 8).  The reference is pure Python:
 * its only "native" entry points on this path are the numba @njit kernels and the numpy/torch
 * calls listed next to each function below (paths relative to /root/reference).  A maintainer
 * binds these symbols with ctypes (INTEGRATION.md shows the stubs) in place of those call sites.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes; no torch / C++ types.
 *  - Every data pointer is a DEVICE (HBM) pointer unless its name ends in `_host`.
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Calls are asynchronous
 *    on that stream; nothing here allocates, frees or synchronises (graph-capture safe) except
 *    the tsm_mem_* / tsm_stream_sync helpers.
 *  - Return value: 0 = TSM_OK, otherwise a TSM_ERR_* code; tsm_last_error() returns a
 *    thread-local message.  The Python host maps TSM_ERR_INVALID -> ValueError,
 *    TSM_ERR_MALFORMED_BUFFER -> MalformedBufferError (tianshou/data/buffer/buffer_base.py:380),
 *    others -> RuntimeError.
 *  - Device layout ("joint-step lanes"): time-major SoA
 *      field[slot][env][agent][...]   slot in [0, sub_size), env in [0, buffer_num)
 *    so that the (env, agent) lane index is the fastest-varying dimension of every per-step scalar.
 *    Reference flat buffer index  <->  (env, slot):  index = env * sub_size + slot
 *    (tianshou/data/buffer/manager.py:38-46, vecbuf.py:35).
 *  - dtypes: payload f32, actions i32, flags u8 (0/1), indices/counters i64, episode-return
 *    accumulators f64 (the reference keeps rew/ep_return in f64, buffer_base.py:377,484).
 */
#ifndef TSMARL_H
#define TSMARL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TSM_ABI_VERSION 4  /* 4: tsm_rollout_tag_desc.vnext_store, TSM_MAX_GATHER_FIELDS 12, tsm_random_permutations_advance; 3: tsm_slab_seg.frag_image, tsm_critic_rows_grad_*(w1_image), tsm_kernel_option_* */

enum {
    TSM_OK = 0,
    TSM_ERR_INVALID = 1,          /* bad argument (ValueError) */
    TSM_ERR_HIP = 2,              /* HIP runtime / launch failure */
    TSM_ERR_MALFORMED_BUFFER = 3, /* buffer_base.py:380-386 */
    TSM_ERR_UNSUPPORTED = 4
};
/* In front of a prototype: this int is a result, not a TSM_* status.  Expands to nothing; the Python binding reads it (with the
 * return types other than int) to know which calls carry a value back instead of raising on non-zero. */
#define TSM_VALUE

TSM_VALUE int tsm_abi_version(void);
const char *tsm_last_error(void);
/* name_out: >= 64 bytes.  Fails with TSM_ERR_HIP when no gfx950 device is visible. */
int tsm_device_info(int *n_cu, int *wave_size, int64_t *hbm_bytes, char *name_out);

/* Kernel selection options.  Where one entry point has two kernels behind it the choice is a rule over the problem size; an
 * option overrides the rule for this process.  Default: the environment variable (read at first use); tsm_kernel_option_set
 * replaces it at any time (hosts that cache launches -- hipGraphs -- key them by the option values).  No reference counterpart.
 *   "actor_tile"   0 = by minibatch size | 32 | 64 (tsm_ppo_actor_rows_update / _grid)            TSM_ACTOR_TILE
 *   "split_bf16"   0 | 1 = layer 1 of tsm_critic_rows_forward on the bf16 matrix pipe, three-way split operands, f32
 *                  accumulation (experimental, never the default)                                   TSM_SPLIT_BF16
 *   "rollout_form" tsm_rollout_spread / tsm_rollout_spread_actor: 0 = by rule | 1 = tile form | 2 = wave-autonomous form   TSM_ROLLOUT_FORM */
int tsm_kernel_option_get(const char *name, int32_t *value_out);
int tsm_kernel_option_set(const char *name, int32_t value);

/* memory / stream helpers for hosts that do not bring their own allocator (PyTorch does) */
int tsm_mem_alloc(void **dptr, int64_t bytes);
int tsm_mem_free(void *dptr);
int tsm_mem_h2d(void *dst, const void *src_host, int64_t bytes, void *stream);
int tsm_mem_d2h(void *dst_host, const void *src, int64_t bytes, void *stream);
int tsm_mem_set(void *dst, int value, int64_t bytes, void *stream);
int tsm_stream_sync(void *stream);
/* Ends a hipGraph capture that failed half-way on `stream` (drops the partial graph); returns 1 if one was ended, else 0. */
TSM_VALUE int tsm_stream_abort_capture(void *stream);

/* ---------------------------------------------------------------------------------------------
 * GAE  [SURVEY 8a: a11, a12]
 * Replaces  Algorithm.compute_episodic_return + value_mask + numba `_gae`
 *           (tianshou/algorithm/algorithm_base.py:631-717, 1079-1134)
 *           and the return_scaling arithmetic of a2c.py:132-146.
 * One independent series per lane; inputs/outputs are [T][n_lane] time-major.
 *   v_next' = v_s_next * v_scale * !terminated;  v' = v_s * v_scale
 *   end     = terminated | truncated | (row is the lane's last row)      (unfinished_index forcing)
 *   delta = rew + gamma*v_next' - v';  adv_t = delta_t + gamma*lambda*(1-end_t)*adv_{t+1}  (f64)
 *   adv_out = f32(adv);  returns_out = f32((adv + v') / v_scale)
 * env_len / env_start (nullable, [n_lane / lanes_per_env] i32): ragged / rotated sub-buffers --
 *   lane rows are slots (start + k) % T for k in [0, len); rows outside are left untouched.
 * terminated / truncated: u8 [T][n_lane] when flags_per_lane != 0, else [T][n_lane/lanes_per_env].
 * ------------------------------------------------------------------------------------------- */
int tsm_gae_lanes(const float *v_s, const float *v_s_next, const float *rew,
                  const uint8_t *terminated, const uint8_t *truncated, int flags_per_lane,
                  int64_t T, int64_t n_lane, int64_t lanes_per_env, const int32_t *env_start,
                  const int32_t *env_len, double gamma, double gae_lambda, double v_scale,
                  float *returns_out, float *adv_out, void *stream);
/* The same with `return_scaling` statistics that live in HBM (a2c.py:132-146): rms = f64 {mean, var, count} of
 * the reference's RunningMeanStd (utils/statistics.py:68-114); v_scale = sqrt(rms[1] + rms_eps) is read by the
 * kernel, so a captured hipGraph follows the statistics from update to update. */
int tsm_gae_lanes_rms(const float *v_s, const float *v_s_next, const float *rew,
                      const uint8_t *terminated, const uint8_t *truncated, int flags_per_lane,
                      int64_t T, int64_t n_lane, int64_t lanes_per_env, const int32_t *env_start,
                      const int32_t *env_len, double gamma, double gae_lambda, const double *rms,
                      double rms_eps, float *returns_out, float *adv_out, void *stream);
/* The few-lanes / long-series form of tsm_gae_lanes (n_lane <= 64, T >= 1024: the MARL trainers' one time-ordered lane of
 * n_env * T rows, training_coordinator.py:118,154,336) runs its super-chunks of 4096 steps on different workgroups when the
 * host has registered a ZEROED device workspace of tsm_gae_scan_workspace_bytes() bytes for the CURRENT device (one per device;
 * the memory stays the caller's; nullptr withdraws it): same bits as the one-workgroup-per-lane form, 12 800 rows 27 -> 9 us.
 * The workspace is cut into slots -- one per eager stream, one per launch recorded into a hipGraph -- so launches in flight never
 * share hand-over state; without a free slot, or on a device without a workspace, the one-workgroup form runs.
 * tsm_gae_set_scan_error_word: a word of PINNED host memory that a scan whose bounded wait ran out sets to 1 (its outputs are NaN
 * from there on); the host reads it where it reads its statistics. */
int64_t tsm_gae_scan_workspace_bytes(void);
int tsm_gae_set_scan_workspace(void *workspace, int64_t bytes);
int tsm_gae_set_scan_error_word(int32_t *host_pinned);

/* RunningMeanStd.update (utils/statistics.py:97-114) with the UNNORMALISED returns of a2c.py:144-146:
 * x[i] = returns[ids ? ids[i] : i] * sqrt(rms[1] + rms_eps), i < n; batch mean / population variance in f64
 * (two-level fixed-order sums of x - x[0]), then the parallel-variance merge into rms = {mean, var, count} in place.
 * work: f64[tsm_rms_update_work_elems(n)]. */
int64_t tsm_rms_update_work_elems(int64_t n);
int tsm_rms_update(const float *returns, const int64_t *ids, int64_t n, double *rms, double rms_eps,
                   double *work, void *stream);

/* `episode_mc_return_to_go` (algorithm_base.py:1137-1151) over n_lane independent episodes
 * stored [T][n_lane]; out f32. */
int tsm_mc_return_to_go_lanes(const float *rew, int64_t T, int64_t n_lane, double gamma,
                              float *out, void *stream);

/* Several row-gathers with element conversion in ONE launch: field k copies n_rows rows of `width` elements,
 *   dst[r][c] = convert(src[src_row(r) * src_row_stride + src_offset + c]),
 * src_row(r) = r (T == 0) or, with T > 0 and n_rows == T * E, the time-major slot of env-major row r = e * T + t:
 * src_row = t * E + e -- the reference's flat index order (manager.py:131-193) read out of a [T][E][...] store; src_offset
 * picks an agent's column of a joint row.  Kinds: f32 -> f32; i32 / i64 / u8 -> i32 / i64 / f32 / u8 (u8: 0 / 1, torch.bool's
 * storage).  Replaces the per-field torch copies of the MARL trainers' per-agent batches (training_coordinator.py:118,154,336) and
 * of learn()'s static buffers.  No reference counterpart. */
#define TSM_MAX_GATHER_FIELDS 12
enum { TSM_KIND_F32 = 0, TSM_KIND_I32 = 1, TSM_KIND_I64 = 2, TSM_KIND_U8 = 3 };
typedef struct tsm_gather_field {
    const void *src;
    void *dst;
    int64_t n_rows;
    int64_t T, E;
    int64_t src_row_stride, src_offset;   /* in elements of the source type */
    int32_t width, src_kind, dst_kind, _pad;
} tsm_gather_field;
int tsm_gather_fields(const tsm_gather_field *fields_host, int32_t n_fields, void *stream);

/* V(obs_next) (a2c.py:124) without a second critic pass over every row.  Rows written by a Collector are chained:
 * obs_next of slot t is obs of slot t + 1 unless the episode ended at t (collector.py:1040-1069), so for T unrotated,
 * equally filled slots of U units (lanes, or joint rows for a centralized critic)
 *   v_next[t][u] = v_s[t + 1][u] (t < T - 1),  v_last[u] = V(obs_next of the last slot) (t = T - 1)
 * provided no episode ended before the last slot: *flag == 0, flag = tsm_any_nonzero_u8(done[0 .. T-1)).  If one did,
 * v_next = v_full, the complete pass (run it with tsm_mlp_forward_cond on the same flag).  Bit-identical to the full
 * pass either way (the critic's rows are computed independently of each other). */
int tsm_any_nonzero_u8(const uint8_t *x, int64_t n, int32_t *flag_out, void *stream);
int tsm_value_next_select(const float *v_s, const float *v_last, const float *v_full, const int32_t *flag, int64_t T,
                          int64_t U, float *v_next_out, void *stream);
/* The same for ENV-major rows [E][T][U] (flat reference index order, sample_indices(0): what the MARL trainers' per-agent
 * batches hold): v_next[e][t][u] = v_s[e][t + 1][u] (t < T - 1), v_last[e][u] (t = T - 1), or v_full when *flag != 0. */
int tsm_value_next_select_env_major(const float *v_s, const float *v_last, const float *v_full, const int32_t *flag,
                                    int64_t E, int64_t T, int64_t U, float *v_next_out, void *stream);
/* V(obs_next) for a buffer that does not store obs_next (ReplayBuffer(ignore_obs_next=True), buffer_base.py:612-616: obs_next
 * is read as obs[next(index)], and next(index) is the row itself at an episode end and at the newest row): for T unrotated,
 * equally filled slots v_next[t][u] = (t == T - 1 || done[t][u / lanes_per_env]) ? v_s[t][u] : v_s[t + 1][u].
 * v_s, v_next_out f32 [T][U]; done u8 [T][U / lanes_per_env]. */
int tsm_value_next_index(const float *v_s, const uint8_t *done, int64_t T, int64_t U, int64_t lanes_per_env,
                         float *v_next_out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * VectorReplayBuffer  [a8, a9]
 * Replaces  ReplayBufferManager.add / _update_state_pre_add / sample_indices(0) /
 *           unfinished_index / _prev_index / _next_index / reset
 *           (tianshou/data/buffer/manager.py:70-229,306-358; buffer_base.py:292-410,495-531;
 *            vecbuf.py:33-37).
 * `state` is one device allocation of tsm_vrb_state_bytes() bytes owned by the caller:
 *   i64 insertion_idx[B], size[B], ep_len[B], ep_start_idx[B], last_index[B], lengths[B];
 *   f64 ep_return[B][rew_dim];  i64 error_flag[1]
 * ------------------------------------------------------------------------------------------- */
int64_t tsm_vrb_state_bytes(int64_t buffer_num, int64_t rew_dim);
int tsm_vrb_init(void *state, int64_t buffer_num, int64_t sub_size, int64_t rew_dim, void *stream);
int tsm_vrb_reset(void *state, int64_t buffer_num, int64_t sub_size, int64_t rew_dim,
                  int keep_statistics, void *stream);

/* One payload field scattered by tsm_vrb_add: row r of `src` ([R][row_bytes], the vector env's
 * AoS step output) goes to `dst` + ((slot * buffer_num + env) * row_bytes)  (time-major SoA). */
typedef struct {
    const void *src;
    void *dst;
    int64_t row_bytes;
} tsm_field;

/* add(): R rows, row r belongs to sub-buffer buffer_ids[r] (NULL = arange(R)); ids must be unique
 * within one call (the reference's Collector never repeats an env id within a step).
 *   rew [R][rew_dim] f32, done [R] u8 (= terminated | truncated, manager.py:150).
 *   done_store: u8 [sub_size][buffer_num] (read by prev/next/unfinished_index).
 * Outputs [R]: ptr (flat reference index env*sub_size+slot), ep_rew [R][rew_dim] f64, ep_len,
 * ep_idx -- the reference's 4-tuple (manager.py:193).  MalformedBufferError is reported through
 * state.error_flag (checked by tsm_vrb_check). */
int tsm_vrb_add(void *state, int64_t buffer_num, int64_t sub_size, int64_t rew_dim,
                const int64_t *buffer_ids, int64_t R, const float *rew, const uint8_t *done,
                uint8_t *done_store, const tsm_field *fields_host, int n_fields, int64_t *ptr_out,
                double *ep_rew_out, int64_t *ep_len_out, int64_t *ep_idx_out, void *stream);
/* synchronises `stream`; returns TSM_ERR_MALFORMED_BUFFER if any add() tripped buffer_base.py:380 */
int tsm_vrb_check(void *state, int64_t buffer_num, int64_t rew_dim, void *stream);

/* sample_indices(0): out [buffer_num*sub_size] i64 (first *n_out valid), env-major, time-ordered.
 * n_out: device i64[1].  scratch: device i64[buffer_num + 1]. */
int tsm_vrb_sample_indices_all(const void *state, int64_t buffer_num, int64_t sub_size,
                               int64_t *out, int64_t *n_out, int64_t *scratch, void *stream);
/* unfinished_index(): out [buffer_num] i64 (first *n_out valid, ascending env order). */
int tsm_vrb_unfinished_index(const void *state, int64_t buffer_num, int64_t sub_size,
                             const uint8_t *done_store, int64_t *out, int64_t *n_out, void *stream);
int tsm_vrb_prev(const void *state, int64_t buffer_num, int64_t sub_size, const uint8_t *done_store,
                 const int64_t *index, int64_t n, int64_t *out, void *stream);
int tsm_vrb_next(const void *state, int64_t buffer_num, int64_t sub_size, const uint8_t *done_store,
                 const int64_t *index, int64_t n, int64_t *out, void *stream);
/* gather rows by flat reference index (ReplayBuffer.__getitem__, buffer_base.py:591-635):
 * out[i] = store[(slot*buffer_num + env)] for index[i] = env*sub_size + slot. */
int tsm_vrb_gather(const void *store, int64_t buffer_num, int64_t sub_size, int64_t row_bytes,
                   const int64_t *index, int64_t n, void *out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Agent dispatch  [a5, a10]
 * Replaces  `np.nonzero(batch.obs.agent_id == agent_id)[0]` per agent and the scatter
 *           `holder.act[agent_index] = act`  (tianshou/algorithm/multiagent/marl.py:148,170-180,233).
 * agent_id [B] i32 in [0, n_agent).  index_out [B] i64: rows of agent 0 (ascending), then agent 1 ...
 * offsets_out [n_agent+1] i64.  scratch: i64 [n_agent * n_blocks + 1], n_blocks = ceil(B/1024).
 * ------------------------------------------------------------------------------------------- */
int tsm_agent_index(const int32_t *agent_id, int64_t B, int32_t n_agent, int64_t *index_out,
                    int64_t *offsets_out, int64_t *scratch, void *stream);
/* dst[index[i]] = src[i]  /  dst[i] = src[index[i]]   rows of row_bytes */
int tsm_scatter_rows(const void *src, const int64_t *index, int64_t n, int64_t row_bytes, void *dst,
                     void *stream);
int tsm_gather_rows(const void *src, const int64_t *index, int64_t n, int64_t row_bytes, void *dst,
                    void *stream);

/* ---------------------------------------------------------------------------------------------
 * Categorical policy head  [a7, a13]
 * Replaces  torch.distributions.Categorical(logits=...).sample / log_prob / entropy
 *           (tianshou/utils/net/discrete.py:22-24; reinforce.py:183-189; ppo.py:160,187,210).
 * logits [B][A] f32 row-major.  Sampling uses a counter-based Philox4x32-10 stream keyed by
 * (seed, offset + row): reproducible, order-independent, NOT bit-identical to torch's CPU RNG.
 * deterministic != 0 -> dist.mode (argmax) (reinforce.py:185-189).  offset_dev (nullable, device u64[1]) is
 * added to `offset`, so that a captured hipGraph advances the stream from device memory.
 * ------------------------------------------------------------------------------------------- */
int tsm_categorical_sample(const float *logits, int64_t B, int32_t A, uint64_t seed,
                           uint64_t offset, const uint64_t *offset_dev, int deterministic, int32_t *act_out,
                           float *logp_out, void *stream);
int tsm_categorical_logp_entropy(const float *logits, const int32_t *act, int64_t B, int32_t A,
                                 float *logp_out, float *ent_out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * PPO clip loss, forward + backward w.r.t. logits and value  [a14]
 * Replaces  the body of PPO._update_with_batch (tianshou/algorithm/modelfree/ppo.py:182-211)
 *           between the network forward and optim.step.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    double eps_clip;    /* 0.2 */
    double dual_clip;   /* <= 0: off */
    double vf_coef;     /* 0.5 */
    double ent_coef;    /* 0.01 */
    int32_t value_clip; /* 0 */
    int32_t adv_norm;   /* 1 */
    /* 0: PPO clip objective (ppo.py:182-211).  1: plain policy gradient, actor_loss = -mean(log_prob * adv), the
     * actor term of A2C (a2c.py:260-270: + vf_coef * mse(returns, value) - ent_coef * entropy, no clipping) and, with
     * vf_coef = ent_coef = 0 and adv = returns, the whole loss of Reinforce (reinforce.py:373-379).  eps_clip,
     * dual_clip, value_clip and logp_old are ignored for kind 1.
     * 2 (tsm_ppo_loss_fwd_bwd only): the VALUE term alone -- vf_coef * value loss, d loss / d value; logits, act,
     * logp_old, adv, adv_stats and dlogits_out may be NULL (the policy terms of the same samples come from
     * tsm_ppo_actor_rows_update). */
    int32_t loss_kind;
    /* <= 1: one critic value per sample.  N > 1 (tsm_ppo_loss_fwd_bwd only): centralized critic -- samples
     * i = r * N + a of a minibatch are the N agents of joint row r, `value` holds one entry per ROW (value[i / N]) and
     * dvalue_out [M / N] receives the sum of the row's N per-sample gradients (M % N == 0). */
    int32_t value_group;
} tsm_ppo_cfg;

/* Per-minibatch advantage statistics (ppo.py:185, torch unbiased std).  Minibatch k covers
 * perm[mb_start[k] .. mb_start[k+1]) (perm == NULL: identity; mb_start: device i64[n_mb+1]).
 * stats_out [n_mb][2] f32 = {mean, std}.  One launch serves every minibatch of an epoch. */
int tsm_ppo_adv_stats(const float *adv, const int64_t *perm, const int64_t *mb_start,
                      int32_t n_mb, float *stats_out, void *stream);
/* The statistics above AND the minibatches' rows, gathered once per update, in ONE launch (minibatches of up to 8192 rows:
 * max_rows >= the longest one, host knowledge).  packed_out receives one record per 16-row tile, tiles in order within a
 * minibatch, minibatch k's first record at index tile_start[k] (device i64[n_mb], in records; minibatch k takes
 * ceil(rows / 16) of them).  A record is tsm_ppo_packed_record_elems(obs_dim) = 16 * obs_dim + 80 four-byte words:
 * obs rows [16][obs_dim] | act[16] (i32) | logp_old[16] | adv[16] | returns[16] | v_old[16]; rows past the end of a ragged
 * last tile are zero.  v_old: v_s_old when the loss clips the value, else returns (any readable array of the same length).
 * stats_out is nullable (no advantage normalisation: rows only).  tsm_ppo_update_fused_packed reads the records. */
int64_t tsm_ppo_packed_record_elems(int32_t obs_dim);
int tsm_ppo_pack_minibatches(const float *adv, const int64_t *perm, const int64_t *mb_start, int32_t n_mb,
                             int64_t max_rows, float *stats_out, const float *obs, int32_t obs_dim,
                             const int32_t *act, const float *logp_old, const float *returns, const float *v_old,
                             const int64_t *tile_start, float *packed_out, void *stream);
/* The same statistics for long minibatches: every 8192-row chunk of a minibatch is reduced by its own workgroup
 * (shifted f64 sums), a second launch folds the chunks in chunk order (deterministic; independent of the grid).
 * max_rows >= the longest minibatch (host knowledge: mb_start lives in HBM); a longer minibatch gets {NaN, NaN};
 * work: f64[tsm_ppo_adv_stats_work_elems]. */
int64_t tsm_ppo_adv_stats_work_elems(int32_t n_mb, int64_t max_rows);
int tsm_ppo_adv_stats_wide(const float *adv, const int64_t *perm, const int64_t *mb_start, int32_t n_mb,
                           int64_t max_rows, double *work, float *stats_out, void *stream);

/* Env-sharded replicas: the advantage normalisation of ppo.py:184-186 over the GLOBAL minibatch (the union
 * of the ranks' parts).  pack: stats [n_mb][2] = this rank's {mean, unbiased std} and its row counts mb_start[k+1] -
 * mb_start[k] -> pack_out f64 [n_mb][3] = {n, sum x, sum x^2}; the caller sums pack over the ranks (one all-reduce
 * for every minibatch of the update); unpack: summed pack -> stats_out [n_mb][2] = {mean, unbiased std} of the union.
 * A part of one row packs {1, m, m^2} (its std is NaN), an empty part {0, 0, 0}; a union of one row has std NaN. */
int tsm_ppo_adv_stats_pack(const float *stats, const int64_t *mb_start, int32_t n_mb, double *pack_out, void *stream);
int tsm_ppo_adv_stats_unpack(const double *pack, int32_t n_mb, float *stats_out, void *stream);

/* One minibatch of M samples: sample i is row perm[i] of the full-batch arrays (perm == NULL:
 * row first_row + i).  logits [M][A] and value [M] are minibatch-contiguous network outputs.
 * Outputs: dlogits [M][A], dvalue [M] (already scaled by 1/M and the coefficients, i.e. d loss),
 * partial [n_blocks(M)][4] f64 per-block sums {clip_obj, vf, ent, 0}; tsm_ppo_loss_finalize
 * folds them into scalars_out[4] = {loss, clip_loss, vf_loss, ent_loss}. */
int64_t tsm_ppo_loss_partial_elems(int64_t M);
int tsm_ppo_loss_fwd_bwd(const float *logits, const float *value, const int32_t *act,
                         const float *logp_old, const float *adv, const float *returns,
                         const float *v_s_old, const int64_t *perm, int64_t first_row, int64_t M,
                         int32_t A, const float *adv_stats, const tsm_ppo_cfg *cfg_host,
                         float *dlogits_out, float *dvalue_out, double *partial_out, void *stream);
int tsm_ppo_loss_finalize(const double *partial, int64_t M, const tsm_ppo_cfg *cfg_host,
                          float *scalars_out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Optimizer step  [a15]
 * Replaces  Algorithm.Optimizer.step: clip_grad_norm_ + torch.optim.Adam.step
 *           (tianshou/algorithm/algorithm_base.py:485-498; optim.py:91-111) on one flat f32
 *           parameter vector (actor+critic union, utils/net/common.py:461-474).
 * grad_slabs [n_slab][n] f32: per-workgroup partial gradients, summed here in slab order
 * (deterministic).  max_grad_norm <= 0: no clipping; otherwise work: f32[tsm_adam_work_elems(n)] device.
 * param_image / image_map (nullable): padded LDS-layout copy of the parameters kept in sync for the fused
 * MLP kernels (tsm_policy_image_elems / tsm_policy_image_map).
 * step: 1-based Adam step count; when step_dev (device i64[1]) is given it overrides `step`.
 * lr_dev (nullable, device f64[1]) overrides `lr`: the learning rate an LR scheduler steps after every update
 * (algorithm_base.py:626-627, optim.py:22-46) lives in HBM, so a captured hipGraph follows the schedule.
 * ------------------------------------------------------------------------------------------- */
/* out[i] = scale * sum_s grad_slabs[s][i]: the flat gradient handed to the RCCL all-reduce of the
 * env-sharded data-parallel path (no reference counterpart: the reference has no distributed backend). */
int tsm_reduce_slabs(const float *grad_slabs, int32_t n_slab, int64_t n, double scale, float *out,
                     void *stream);
int64_t tsm_adam_work_elems(int64_t n);
int tsm_adam_step(float *param, const float *grad_slabs, int32_t n_slab, int64_t n, float *exp_avg,
                  float *exp_avg_sq, int64_t step, const int64_t *step_dev, double lr, const double *lr_dev,
                  double beta1, double beta2, double eps, double weight_decay, double max_grad_norm, float *work,
                  float *param_image, const int32_t *image_map, void *stream);
/* Segmented forms: the flat vector is covered, in order, by up to TSM_MAX_SLAB_SEGS segments whose gradients come from
 * different kernels (tsm_ppo_actor_rows_update / tsm_ppo_critic_rows_update write separate slab arrays): the gradient of
 * parameter offset + i, i < n, in slab s is slabs[s * stride + i].  One launch for the whole vector; with
 * max_grad_norm > 0 one reduction launch in front and ONE norm over all segments (clip_grad_norm_ over
 * ActorCritic.parameters(), algorithm_base.py:485-498). */
#define TSM_MAX_SLAB_SEGS 6
typedef struct tsm_slab_seg {
    const float *slabs;
    int64_t offset, n, stride;
    int32_t n_slab;
    int32_t frag_k1;        /* with frag_image: the segment is a row-major [128][frag_k1] first-layer weight matrix */
    const float *scale_dev; /* nullable device f32[1]: the segment's summed gradient is multiplied by it (a loss whose
                               gradient is a device-side scalar times a sum, e.g. CTDEPolicy's actor loss, ctde.py:185) */
    float *frag_image;      /* nullable: the updated parameters are ALSO stored in the fragment order the one-launch critic
                               kernels load with coalesced 16-B loads (tsm_critic_rows_w1_image: same layout), so the
                               next gradient step need not gather W1 through 64-B pieces of 1.5 KB rows */
    int32_t frag_kj, _pad;  /* k-groups of 16 per image row: tsm_critic_rows_w1_image_kj(frag_k1) */
} tsm_slab_seg;
int tsm_reduce_slabs_segs(const tsm_slab_seg *segs_host, int32_t n_seg, int64_t n, double scale, float *out,
                          void *stream);
int tsm_adam_step_segs(float *param, const tsm_slab_seg *segs_host, int32_t n_seg, int64_t n, float *exp_avg,
                       float *exp_avg_sq, int64_t step, const int64_t *step_dev, double lr, const double *lr_dev,
                       double beta1, double beta2, double eps, double weight_decay, double max_grad_norm, float *work,
                       void *stream);
/* param_image[image_map[i]] = param[i]  (initial fill of the padded image; pads must already be zero) */
int tsm_scatter_image(const float *param, int64_t n, const int32_t *image_map, float *param_image,
                      void *stream);

/* ---------------------------------------------------------------------------------------------
 * Fused actor + critic MLP (f32 MFMA)  [a7, a11, a13, a14]
 * Networks: obs[D] -> Linear(H) ReLU -> Linear(H) ReLU -> {Linear(A) logits | Linear(1) value},
 * i.e. Net(hidden_sizes=[H,H]) + DiscreteActor(softmax_output=False) / DiscreteCritic with separate
 * trunks (tianshou/utils/net/common.py:246-369, discrete.py:27-124).  `params` is ONE flat f32 vector
 * in ActorCritic.parameters() order (common.py:461-474):
 *   actor W1[H][D] b1[H] W2[H][H] b2[H] W3[A][H] b3[A] | critic W1[H][D] b1[H] W2[H][H] b2[H] W3[1][H] b3[1]
 * Supported: H == 64, D <= 64, A <= 16 (others: TSM_ERR_INVALID).
 *
 * tsm_policy_forward replaces ProbabilisticActorPolicy.forward + critic(obs) + dist.log_prob
 * (reinforce.py:167-192, a2c.py:121-127, ppo.py:157-161) for obs [B][D]:
 *   mode 0: logits/value only;  1: sample (Philox, key=seed, counter=offset+row);  2: dist.mode;
 *   mode 3: log-prob of the GIVEN actions act_io.   logits_out/value_out/logp_out are nullable.
 *   offset_dev (nullable, device u64[1]) is added to `offset`: lets a captured hipGraph advance the
 *   sampling counter from device memory (tsm_mpe_spread_step bumps it).
 *
 * tsm_ppo_update_fused replaces one gradient step of PPO._update_with_batch (ppo.py:182-212) up to the
 * parameter gradients: network forward, loss (as tsm_ppo_loss_fwd_bwd) and the whole backward pass.
 * Sample i of the minibatch is row perm[i] (perm == NULL: first_row + i) of obs [n][D], act, logp_old,
 * adv, returns, v_s_old.  Each of the n_blocks workgroups writes one gradient slab:
 * grad_slabs_out [n_blocks][P]; feed them to tsm_adam_step(n_slab = n_blocks).
 * loss_partial_out: f64 [n_blocks][4]; scalars_out (nullable) f32[4] = {loss, clip, vf, ent}.
 * opt_step_dev (nullable, device i64[1]): incremented by one per call -- the device-resident optimizer
 * step count that tsm_adam_step(step_dev=...) reads, so a captured hipGraph can be replayed.
 * ------------------------------------------------------------------------------------------- */
int64_t tsm_policy_param_count(int32_t obs_dim, int32_t hidden, int32_t n_act);
/* Padded parameter image: the exact LDS layout of both nets (zero pads included).  When `param_image` is
 * given to the kernels below they stage it with straight 16-B copies instead of re-packing `params`. */
int64_t tsm_policy_image_elems(int32_t obs_dim, int32_t hidden, int32_t n_act);
int tsm_policy_image_map(int32_t obs_dim, int32_t hidden, int32_t n_act, int32_t *map_out_host);
int tsm_policy_forward(const float *params, const float *param_image, int32_t obs_dim, int32_t hidden,
                       int32_t n_act,
                       const float *obs, int64_t B, int mode, uint64_t seed, uint64_t offset,
                       const uint64_t *offset_dev, float *logits_out, float *value_out, int32_t *act_io, float *logp_out,
                       void *stream);
/* recommended n_blocks (= number of gradient slabs; the launch is n_blocks x 2 workgroups, one net each) for a
 * minibatch of M rows.  NOT monotone in M (a slab is 45 KB written here and read back by tsm_adam_step, so past a full
 * chip fewer slabs with two tiles each are faster): when one workspace serves minibatches of several sizes, size
 * grad_slabs_out / loss_partial_out by the LARGEST value over those sizes, not by the value at the largest size.
 * tsm_ppo_update_fused writes n_blocks * n_param floats and n_blocks * 4 doubles. */
TSM_VALUE int tsm_ppo_update_grid(int64_t M, int32_t max_blocks);
int tsm_ppo_update_fused(const float *params, const float *param_image, int32_t obs_dim, int32_t hidden,
                         int32_t n_act,
                         const float *obs, const int32_t *act, const float *logp_old, const float *adv,
                         const float *returns, const float *v_s_old, const int64_t *perm,
                         int64_t first_row, int64_t M, const float *adv_stats,
                         const tsm_ppo_cfg *cfg_host, int32_t n_blocks, float *grad_slabs_out,
                         double *loss_partial_out, float *scalars_out, int64_t *opt_step_dev,
                         void *stream);
/* The same step with the minibatch's rows also given as tile records (`packed`: the minibatch's first record, as written by
 * tsm_ppo_pack_minibatches from these very arrays and this perm): the kernel reads its tile's record in the same batch of loads
 * as the weight image instead of row ids first and the rows behind them.  Same bits.  packed == NULL, or no param_image: the
 * rows are read through perm / first_row, which must describe them either way. */
int tsm_ppo_update_fused_packed(const float *params, const float *param_image, int32_t obs_dim, int32_t hidden,
                                int32_t n_act,
                                const float *obs, const int32_t *act, const float *logp_old, const float *adv,
                                const float *returns, const float *v_s_old, const int64_t *perm,
                                int64_t first_row, int64_t M, const float *adv_stats,
                                const tsm_ppo_cfg *cfg_host, int32_t n_blocks, float *grad_slabs_out,
                                double *loss_partial_out, float *scalars_out, int64_t *opt_step_dev,
                                const float *packed, void *stream);

/* Loss statistics of many gradient steps in ONE launch (pass scalars_out = NULL to tsm_ppo_update_fused):
 * step k reads loss partials at partial + k*stride_elems (n_blocks_dev[k] rows of 4 f64) and M_dev[k];
 * scalars_out f32 [n_steps][4] = {loss, clip_loss, vf_loss, ent_loss} (the 4 .item() of ppo.py:213-216). */
int tsm_ppo_finalize_many(const double *partial, int64_t stride_elems, const int32_t *n_blocks_dev,
                          const int64_t *M_dev, int32_t n_steps, const tsm_ppo_cfg *cfg_host,
                          float *scalars_out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Batched MPE worlds  [SURVEY 8f-1; replaces the per-env Python loop of a1-a3 for simple_spread]
 * Device-resident restatement of PettingZoo-MPE simple_spread behind the parallel-mode
 * EnhancedPettingZooEnv data formats (tianshou/env/enhanced_pettingzoo_env.py:130-222) and the
 * BaseVectorEnv.step/reset contract (tianshou/env/venvs.py:195-322).  pettingzoo's sources are not in
 * the reference tree: dynamics parity is UNPINNED.  State (caller-owned, device):
 *   agent_pos, agent_vel, landmark_pos f32 [n_env][N][2]; steps i32 [n_env]; episode_ctr u64 [n_env].
 * obs layout per agent (6N): [vel(2), pos(2), landmarks rel (2N), others rel (2(N-1)), comm (2(N-1))].
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t n_env, n_agent, max_cycles, _pad;
    double dt, damping, contact_force, contact_margin, agent_size, landmark_size, accel, max_speed,
        local_ratio;
} tsm_mpe_cfg;

/* env_ids NULL: reset every env.  obs_out [n_env][N][6N] (rows of the reset envs are written). */
int tsm_mpe_spread_reset(const tsm_mpe_cfg *cfg_host, uint64_t seed, uint64_t *episode_ctr,
                         const int64_t *env_ids, int64_t n_ids, float *agent_pos, float *agent_vel,
                         float *landmark_pos, int32_t *steps, float *obs_out, void *stream);
/* act i32 [n_env][N] in {0 noop, 1 -x, 2 +x, 3 -y, 4 +y}.  Outputs: obs_next (terminal obs for finished
 * episodes), obs_cur (nullable; what the policy sees next: reset obs where done and auto_reset), rew f32
 * [n_env][N], terminated/truncated u8 [n_env][N], done_env u8 [n_env].  rng_tick (nullable, device
 * u64[1]) += rng_tick_inc once per call. */
int tsm_mpe_spread_step(const tsm_mpe_cfg *cfg_host, uint64_t seed, uint64_t *episode_ctr,
                        const int32_t *act, float *agent_pos, float *agent_vel, float *landmark_pos,
                        int32_t *steps, float *obs_next_out, float *obs_cur_out, float *rew_out,
                        uint8_t *terminated_out, uint8_t *truncated_out, uint8_t *done_env_out,
                        int auto_reset, uint64_t *rng_tick, uint64_t rng_tick_inc, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Persistent rollout  [a4 + a7 + a8 fused; SURVEY 8f-1]
 * One launch == one Collector.collect(n_step = n_steps * n_env) on the batched simple_spread env with a
 * shared actor/critic: policy forward + sample + log-prob + value, env step (+ reset of finished envs),
 * buffer index algebra and payload scatter for n_steps vector steps
 * (tianshou/data/collector.py:854-1069 loop body).  Bit-identical to calling tsm_policy_forward ->
 * tsm_mpe_spread_step -> tsm_vrb_add n_steps times.  Additionally stores vnext = V(obs_next) per row
 * (a2c.py:124), so the update needs no critic pass.  All pointers are device pointers; nullable:
 * params (if param_image given), obs_next_store, logp_store, vs_store, vnext_store, obs_cur_out, offset_dev.
 * Per-step outputs: ptr_out/ep_len_out/ep_idx_out i64 [n_steps][n_env], ep_rew_out f64 [n_steps][n_env][N].
 * The sampling counter of step t, row i is  offset + *offset_dev + t*n_env*N + i  (advance it afterwards
 * with tsm_u64_add).
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    const float *params, *param_image;
    int32_t obs_dim, hidden, n_act, mode; /* mode 1 sample, 2 dist.mode */
    uint64_t policy_seed, offset;
    const uint64_t *offset_dev;
    tsm_mpe_cfg env;
    uint64_t env_seed;
    uint64_t *episode_ctr;
    float *agent_pos, *agent_vel, *landmark_pos;
    int32_t *steps;
    int32_t auto_reset, n_steps;
    float *obs_cur_out;
    void *vrb_state;
    int64_t sub_size;
    uint8_t *done_store;
    float *obs_store, *obs_next_store, *rew_store, *logp_store, *vs_store, *vnext_store;
    int32_t *act_store;
    uint8_t *term_store, *trunc_store;
    int64_t *ptr_out;
    double *ep_rew_out;
    int64_t *ep_len_out, *ep_idx_out;
    /* compact record of the episodes finished during the rollout (nullable; what CollectStats needs, collector.py:
     * 1001-1009, without shipping the dense per-step arrays to the host): i64 words
     *   [n_env] count | [n_env][max_ep] (step << 32 | length) | [n_env][max_ep][N] f64 episode return.
     * count may exceed max_ep (records beyond max_ep are dropped): size max_ep for the worst case. */
    int64_t *ep_rec;
    int32_t max_ep, _pad2;
    /* optional: advance the device-resident sampling counter *offset_dev by offset_inc once every workgroup has read
     * it (done by the last workgroup to finish, counted in *done_ctr: one zero-initialised u32 in HBM that the
     * kernel leaves at zero).  Saves the separate tsm_u64_add launch per collect().  done_ctr NULL = no advance. */
    uint64_t offset_inc;
    uint32_t *done_ctr;
} tsm_rollout_desc;

int tsm_rollout_spread(const tsm_rollout_desc *desc_host, void *stream);
/* tsm_rollout_spread, and on the CUs its workgroups leave idle the draw of the permutations of the update that follows the
 * collect: perm_out [n_perm][perm_n] as tsm_random_permutations(perm_n, n_perm, perm_seed, 0, perm_counter_dev, perm_scale,
 * perm_group_size, perm_offset_mul, perm_out) writes it, bit for bit, without that launch.  *perm_counter_dev is read, never
 * written: whoever advances it today still does.  The ride-along is taken only where the launch is the eight-wave tile form with
 * fewer workgroups than the device has CUs (tsm_rollout_prep_extra > 0); *taken_out (host) says whether: 1 = perm_out is
 * filled behind this launch, 0 = the launch was exactly tsm_rollout_spread's and the caller draws the permutations itself.
 * perm_out NULL (or perm_n / n_perm 0): no request, tsm_rollout_spread.  n_cu: 0 = the device's CU count, else the count the
 * rule is to assume (tests). */
int tsm_rollout_spread_prep(const tsm_rollout_desc *desc_host, int64_t perm_n, int32_t n_perm, uint64_t perm_seed,
                            const uint64_t *perm_counter_dev, int64_t perm_scale, int32_t perm_group_size,
                            int64_t perm_offset_mul, int64_t *perm_out, int32_t n_cu, int32_t *taken_out, void *stream);
/* The rule itself, on the host: *extra_out = the spare workgroups a launch of `tiles` rollout workgroups gets on n_cu CUs for
 * n_perm permutations of perm_n entries -- min(idle CUs, one per 512 entries, 64); 0 = the request is declined. */
int tsm_rollout_prep_extra(int64_t tiles, int32_t n_cu, int64_t perm_n, int32_t n_perm, int32_t *extra_out);
/* The same collect loop for a 128-wide ACTOR (obs -> 128 -> 128 -> 5, e.g. BASELINE configs[2]: N = 8, actor
 * 48-128-128-5 next to a centralized critic that does not fit a CU's LDS): desc.params = the actor's parameters
 * (w0 b0 w1 b1 w2 b2), desc.hidden = 128, param_image unused; vs_store / vnext_store are NOT written -- the update
 * computes V(obs) / V(obs_next) for all rows in two batched passes (a2c.py:121-127).  Everything else as
 * tsm_rollout_spread; results are bit-identical to tsm_mlp_forward -> tsm_categorical_sample -> tsm_mpe_spread_step ->
 * tsm_vrb_add step by step.  Up to eight agents (obs_dim <= 48; TSM_ERR_INVALID above: hosts keep the three-launch loop). */
int tsm_rollout_spread_actor(const tsm_rollout_desc *desc, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Batched simple_tag (predator-prey, two teams)  [(f)1, BASELINE configs[4]]
 * Same role and call shape as tsm_mpe_spread_*: the vector-env step the reference performs per env through
 * EnhancedPettingZooEnv (enhanced_pettingzoo_env.py:175-222) under DummyVectorEnv (venvs.py:237-322), for the
 * grouped-policy / self-play / league configurations (training_coordinator.py:413-747).  Agents are ordered
 * adversaries first (n_adv), then good agents; observations are zero-padded to the common width
 * tsm_mpe_tag_obs_dim() = 4 + 2 n_obst + 2 (n_adv + n_good - 1) + 2 n_good (pettingzoo_env.py:55-67 requires
 * identical spaces).  Dynamics restated from the published MPE spec: parity with pettingzoo unpinned.
 * State: agent_pos/vel [n_env][NA][2], landmark_pos [n_env][n_obst][2].
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t n_env, n_adv, n_good, n_obst, max_cycles, _pad;
    double dt, damping, contact_force, contact_margin;          /* 0.1, 0.25, 100, 1e-3 */
    double adv_size, good_size, obst_size;                       /* 0.075, 0.05, 0.2 */
    double adv_accel, good_accel, adv_speed, good_speed;        /* 3.0, 4.0, 1.0, 1.3 */
} tsm_mpe_tag_cfg;
TSM_VALUE int tsm_mpe_tag_obs_dim(const tsm_mpe_tag_cfg *cfg_host);
int tsm_mpe_tag_reset(const tsm_mpe_tag_cfg *cfg_host, uint64_t seed, uint64_t *episode_ctr,
                      const int64_t *env_ids, int64_t n_ids, float *agent_pos, float *agent_vel,
                      float *landmark_pos, int32_t *steps, float *obs_out, void *stream);
int tsm_mpe_tag_step(const tsm_mpe_tag_cfg *cfg_host, uint64_t seed, uint64_t *episode_ctr, const int32_t *act,
                     float *agent_pos, float *agent_vel, float *landmark_pos, int32_t *steps, float *obs_next_out,
                     float *obs_cur_out, float *rew_out, uint8_t *terminated_out, uint8_t *truncated_out,
                     uint8_t *done_env_out, int auto_reset, uint64_t *rng_tick, uint64_t rng_tick_inc, void *stream);
int tsm_u64_add(uint64_t *counter, uint64_t inc, void *stream);

/* Persistent rollout for simple_tag under GROUPED policies  [a4 + a6 + a7 + a8 fused for BASELINE configs[4]]
 * One launch == one Collector.collect(n_step = n_steps * n_env) on the batched simple_tag env with ONE 64-wide
 * actor/critic per team (FlexibleMultiAgentPolicyManager(mode="grouped"), flexible_policy.py:96-98; collector loop
 * data/collector.py:854-1069): params[0] serves the adversaries (agent columns [0, n_adv)), params[1] the good agents
 * (both flat vectors as for tsm_policy_forward; pass the same pointer twice for one shared policy).  Bit-identical to,
 * per step, tsm_policy_forward on each team's agent-major rows (sampling counter of step t, column a, env e:
 * offset[team] + *offset_dev + t n_env NA + a n_env + e, as MultiAgentPolicy hands a team's columns to its policy)
 * -> tsm_mpe_tag_step -> tsm_vrb_add.  logp_store / vs_store receive each row's own policy outputs (nullable);
 * vnext_store (nullable) V(obs_next) by the row's own team's critic, as tsm_rollout_spread produces it: the next step's V(obs)
 * where the episode goes on, a forward pass of the terminal observation where it ended, a last pass behind the loop for the rows
 * of the final step -- bit-identical to tsm_policy_forward on the stored obs_next rows.  Everything else as tsm_rollout_spread. */
typedef struct {
    const float *params[2];
    uint64_t policy_seed[2], offset[2];
    int32_t mode[2]; /* per team: 1 sample, 2 dist.mode */
    int32_t obs_dim, hidden, n_act;
    int32_t env_major_counter; /* 0: counter a n_env + e inside a step (grouped policies); 1: e NA + a (ONE shared policy
                                * called on the [n_env][NA] rows, params[0] == params[1]) */
    const uint64_t *offset_dev;
    tsm_mpe_tag_cfg env;
    uint64_t env_seed;
    uint64_t *episode_ctr;
    float *agent_pos, *agent_vel, *landmark_pos;
    int32_t *steps;
    int32_t auto_reset, n_steps;
    float *obs_cur_out;
    void *vrb_state;
    int64_t sub_size;
    uint8_t *done_store;
    float *obs_store, *obs_next_store, *rew_store, *logp_store, *vs_store;
    int32_t *act_store;
    uint8_t *term_store, *trunc_store;
    int64_t *ptr_out;
    double *ep_rew_out;
    int64_t *ep_len_out, *ep_idx_out;
    int64_t *ep_rec; /* compact episode record, layout as in tsm_rollout_desc (nullable) */
    int32_t max_ep, _pad2;
    uint64_t offset_inc; /* added to *offset_dev by the last workgroup to finish (done_ctr: zeroed u32 in HBM; NULL = off) */
    uint32_t *done_ctr;
    float *vnext_store; /* [S][n_env][NA] V(obs_next) of every added row (nullable) */
} tsm_rollout_tag_desc;
int tsm_rollout_tag(const tsm_rollout_tag_desc *desc_host, void *stream);

/* ---------------------------------------------------------------------------------------------
 * 128-wide actor, one gradient step in one launch  [a7, a14 at BASELINE configs[2]: actor obs-128-128-A]
 * Replaces the actor half of PPO._update_with_batch (ppo.py:182-212): policy(minibatch).dist, advantage
 * normalisation, ratio / clip / dual-clip surrogate, entropy and the actor's backward pass.  The loss is separable
 * (clip + entropy: actor; value term: critic), so the critic runs beside it: tsm_mlp_forward ->
 * tsm_ppo_loss_fwd_bwd(loss_kind = 2) -> tsm_mlp_backward, and the gradient halves meet in tsm_adam_step.
 * actor_params: w0[H][D] b0[H] w1[H][H] b1[H] w2[A][H] b2[A] (torch parameters() order), H == 128, D <= 64, A <= 16.
 * Sample i of the minibatch is row perm[i] (NULL: first_row + i) of obs [n][D], act, logp_old, adv.
 * Two kernels behind one entry point, picked by M alone (tsm_ppo_actor_rows_grid follows the same rule): 64-sample tiles with the
 * layer-2 weights in registers (csrc/actor_rows64.hip) once every CU gets at least one such tile, 32-sample tiles with all
 * weights in LDS (csrc/ppo_rows.hip) below that; option "actor_tile" = 32 | 64 forces one (tsm_kernel_option_set).
 * n_blocks = tsm_ppo_actor_rows_grid(M) persistent workgroups, each writes ONE gradient slab:
 * grad_slabs_out [n_blocks][tsm_ppo_actor_rows_param_count]; loss_partial_out f64 [n_blocks][4] =
 * {sum clip objective, 0, sum entropy, 0} (the layout tsm_ppo_finalize_many folds).
 * opt_step_dev (nullable, device i64[1]): advanced by one per call, as tsm_ppo_update_fused does.
 * cfg->loss_kind == 1 (policy gradient, obj = logp * adv): logp_old may be NULL, and adv NULL means adv = 1 for every
 * sample -- the launch then yields d(-mean logp)/d params and sum logp (CTDEPolicy.learn's actor term up to the scalar
 * mean(advantage), quirk Q7).
 * ------------------------------------------------------------------------------------------- */
TSM_VALUE int tsm_ppo_actor_rows_supported(int32_t obs_dim, int32_t hidden, int32_t n_act);
/* Raises the dynamic-LDS limit of every instantiation of the actor / critic rows kernels (idempotent, no stream work).  The
 * launch entry points call it themselves; a host that CAPTURES them into a hipGraph calls it once before its first capture. */
int tsm_ppo_rows_init(void);
int64_t tsm_ppo_actor_rows_param_count(int32_t obs_dim, int32_t hidden, int32_t n_act);
TSM_VALUE int tsm_ppo_actor_rows_grid(int64_t M);
int tsm_ppo_actor_rows_update(const float *actor_params, int32_t obs_dim, int32_t hidden, int32_t n_act,
                              const float *obs, const int32_t *act, const float *logp_old, const float *adv,
                              const int64_t *perm, int64_t first_row, int64_t M, const float *adv_stats,
                              const tsm_ppo_cfg *cfg, int32_t n_blocks, float *grad_slabs_out,
                              double *loss_partial_out, int64_t *opt_step_dev, void *stream);

/* The critic of the same configuration in one launch: value = MLP(row) with in_dim = n_agent * obs_dim inputs (centralized
 * critic over the joint row, ctde.py:291-294 "concatenate"; n_agent = 1: a local critic on the sample's own observation),
 * the value term of the PPO loss (ppo.py:198-208) for the n_agent samples row * n_agent + a of every row, and the critic's
 * backward pass.  critic_params: w0[H][in_dim] b0[H] w1[H][H] b1[H] w2[1][H] b2[1], H == 128, in_dim <= 384.
 * Row i of the minibatch is joint row rows[i] (NULL: first_row + i) of obs_rows [n][in_dim]; returns / v_s_old are
 * per-sample arrays.  grad_slabs_out [n_blocks][tsm_ppo_critic_rows_param_count]; loss_partial_out f64 [n_blocks][4] =
 * {0, sum of the value-loss terms, 0, 0}; the mean is over Mr * n_agent samples. */
TSM_VALUE int tsm_ppo_critic_rows_supported(int32_t in_dim, int32_t hidden, int32_t n_agent);
int64_t tsm_ppo_critic_rows_param_count(int32_t in_dim, int32_t hidden);
TSM_VALUE int tsm_ppo_critic_rows_grid(int64_t Mr);
int tsm_ppo_critic_rows_update(const float *critic_params, int32_t in_dim, int32_t hidden, int32_t n_agent,
                               const float *obs_rows, const float *returns, const float *v_s_old, const int64_t *rows,
                               int64_t first_row, int64_t Mr, const tsm_ppo_cfg *cfg, int32_t n_blocks,
                               float *grad_slabs_out, double *loss_partial_out, void *stream);

/* V(row) of the same critic for MANY rows in one launch, activations never leaving the CU  [a7, a11]
 * Replaces  the critic passes of the on-policy preprocessing, `critic(batch.obs)` / `critic(batch.obs_next)`
 *           (tianshou/algorithm/modelfree/a2c.py:121-127, chunked by max_batchsize there), three GEMM launches here before.
 * critic_params: w0[H][in_dim] b0[H] w1[H][H] b1[H] w2[n_out][H] b2[n_out] (H == 128, in_dim <= 384, n_out <= 16); the value
 * of a row is the MEAN of its n_out outputs (CentralizedCritic: one output per agent, averaged by CTDEPolicy.learn,
 * ctde.py:154-157; n_out = 1: the PPO critic).  Row i is rows[i] (NULL: first_row + i) of obs_rows [n][in_dim]; values_out [Mr].  run_if (nullable, device i32[1]): the launch is a no-op when it holds 0 (a pass a
 * captured graph carries for the rows that need it, tsm_value_next_select).  The first layer sums k in a fixed permuted
 * order (csrc/critic_rows.hip): values agree with tsm_mlp_forward to f32 rounding, not bit for bit.
 * tsm_critic_rows_init: one-time function attributes of the instantiation serving in_dim -- call outside stream capture. */
TSM_VALUE int tsm_critic_rows_forward_supported(int32_t in_dim, int32_t hidden);
int tsm_critic_rows_init(int32_t in_dim, int32_t hidden);
int tsm_critic_rows_forward(const float *critic_params, int32_t in_dim, int32_t hidden, int32_t n_out,
                            const float *obs_rows, const int64_t *rows, int64_t first_row, int64_t Mr,
                            const int32_t *run_if, float *values_out, void *stream);

/* One gradient step of the same critic in two launches (second generation of tsm_ppo_critic_rows_update)  [a7, a14, a16]
 * (A) tsm_critic_rows_grad_ppo / _td: forward, loss and backward down to dH1 = d loss / d (layer-1 pre-activation), with
 *     the layer-1 weights resident in registers and the observation tile in LDS (csrc/critic_train.hip).
 *       dh1_out [Mr][128] (minibatch row order); rest_slabs_out [n_blocks][P - 128 in_dim]: the gradients of
 *       b1 | W2 | b2 | W3 | b3 (parameter order), one slab per workgroup; n_blocks = tsm_critic_rows_grad_grid(Mr, td).
 *       _ppo with h1_out / dh2_out (nullable pair, [Mr][128] each): the launch PUBLISHES the layer-1 activations and
 *       d loss / d (layer-2 pre-activation) instead of forming dW2 itself -- the W2 part of every rest slab is then NOT written
 *       (hand the optimizer b1 and b2 | W3 | b3 as views into the slabs, and dW2 from launch (B)).
 *     _ppo  Replaces  the value term of PPO._update_with_batch (ppo.py:198-212) on joint rows, as tsm_ppo_critic_rows_update:
 *           loss_partial_out f64 [n_blocks][4] = {0, sum of the value-loss terms, 0, 0}.
 *     _td   Replaces  values = critic(global_obs).mean(1); values_next = critic(global_obs_next).mean(1);
 *           td_target = rew + discount_factor * values_next * (~terminated); critic_loss = mse_loss(values, td_target);
 *           critic_loss.backward()                   (tianshou/algorithm/multiagent/ctde.py:149-172, 188-190)
 *           for CHAINED rows: the batch is the env-major view [E][T] of a time-major store joint_rows [T][E][in_dim] (store
 *           row t * E + e) and obs_next of (e, t) is obs of (e, t + 1) for t < T - 1 -- its value is the next row's, out of
 *           the same forward pass (a tile owns 31 rows and computes the 32nd as a halo); v_last [E] = values of obs_next of
 *           the last slot (tsm_critic_rows_forward on those E rows).  use_full (nullable device i32[1]) != 0: an episode
 *           ended before the last slot, so rows are not chained there -- every target then takes v_next_full[i] (env-major
 *           [T E]: V(obs_next) of every row, a pass the caller launches under the same flag).  rew / terminated of store row r:
 *           x[r * scalar_stride + scalar_offset] (one agent's column of [T][E][N] arrays).  loss_partial_out =
 *           {sum (td_target - values), sum (values - td_target)^2, 0, 0}: mean advantage / critic_loss after division by T E.
 * (B) tsm_critic_rows_dw1: dW1 = dH1^T X over the same rows as a split-K pass (csrc/critic_dw1.hip):
 *       w1_slabs_out [n_chunks][128 in_dim], n_chunks = tsm_critic_rows_dw1_chunks(Mr, in_dim) partial sums over row chunks.
 *     Row i of the minibatch is rows[i], else (tm_T > 0) store row (i % tm_T) * tm_E + i / tm_T, else first_row + i.
 * The optimizer takes both slab arrays as segments (tsm_adam_step_segs: W1 at offset 0, the rest at offset 128 in_dim).
 * critic_params: w0[H][in_dim] b0 w1[H][H] b1 w2[n_out][H] b2[n_out], H == 128, in_dim <= 384 (a multiple of 4 above 64).
 * w1_image (nullable): w0 in the kernels' FRAGMENT ORDER, [8 waves][kj][64 lanes][4] floats with element (w, j, lane, i) =
 * w0[16 w + lane % 16][16 j + 4 (lane / 16) + i] (zero where the column is >= in_dim), kj = tsm_critic_rows_w1_image_kj(in_dim):
 * every wave then loads its share with 1 KB-coalesced instructions instead of gathering 64-B pieces of sixteen 1.5 KB rows
 * (3.8 us of a 10 us prologue at in_dim = 384).  tsm_critic_rows_w1_image builds it from w0; tsm_adam_step_segs keeps it in
 * step with the parameters (tsm_slab_seg.frag_image).  It must hold the SAME values as critic_params' w0; NULL = gather. */
int64_t tsm_critic_rows_param_count(int32_t in_dim, int32_t hidden, int32_t n_out);
TSM_VALUE int tsm_critic_rows_w1_image_kj(int32_t in_dim);
int64_t tsm_critic_rows_w1_image_elems(int32_t in_dim);
int tsm_critic_rows_w1_image(const float *w0, int32_t in_dim, float *image_out, void *stream);
TSM_VALUE int tsm_critic_rows_grad_grid(int64_t Mr, int32_t td);
int tsm_critic_rows_grad_ppo(const float *critic_params, const float *w1_image, int32_t in_dim, int32_t hidden, int32_t n_agent,
                             const float *obs_rows, const float *returns, const float *v_s_old, const int64_t *rows,
                             int64_t first_row, int64_t Mr, const tsm_ppo_cfg *cfg, int32_t n_blocks, float *dh1_out,
                             float *h1_out, float *dh2_out, float *rest_slabs_out, double *loss_partial_out, void *stream);
int tsm_critic_rows_grad_td(const float *critic_params, const float *w1_image, int32_t in_dim, int32_t hidden, int32_t n_out,
                            const float *joint_rows, int64_t T, int64_t E, const float *rew, const uint8_t *terminated,
                            int64_t scalar_stride, int64_t scalar_offset, const float *v_last, const float *v_next_full,
                            const int32_t *use_full, double gamma, int32_t n_blocks, float *dh1_out,
                            float *rest_slabs_out, double *loss_partial_out, void *stream);
/* The two scalars of CTDEPolicy.learn and the actor gradient's scale from the kernels' partial sums (ctde.py:181-199):
 * critic_partial [nb_c][4] = {sum (td - v), sum (v - td)^2, ..} (tsm_critic_rows_grad_td), actor_partial [nb_a][4] =
 * {sum log_probs, ..} (tsm_ppo_actor_rows_update, loss_kind 1, adv NULL) -> scalars_out[2] = {actor_loss =
 * -mean(log_probs) * mean(advantage), critic_loss}, mean_adv_out[1] = mean(advantage) (the scale_dev of the actor's slab
 * segment).  One workgroup; fixed summation order.  scalars_out may be pinned host memory. */
int tsm_ctde_finalize(const double *critic_partial, int32_t nb_c, const double *actor_partial, int32_t nb_a, int64_t B,
                      float *scalars_out, float *mean_adv_out, void *stream);
TSM_VALUE int tsm_critic_rows_dw1_chunks(int64_t Mr, int32_t in_dim);
/* side (nullable, at most 2): gradient-slab sets of OTHER parameter segments, already complete when this launch starts (the
 * actor step's slabs, the small-gradient slabs of launch (A)), summed to ONE row each by extra workgroups of this launch while
 * its main workgroups wait on their loads: out[i] = sum over slabs of slabs[s * stride + i] in tsm_adam_step's own order, so
 * handing `out` to the optimizer as a one-slab segment gives bit-identical gradients -- and the optimizer launch reads 6 MB
 * instead of 48 (BASELINE configs[2] step). */
typedef struct tsm_slab_reduce {
    const float *slabs;
    int64_t n, stride;
    int32_t n_slab, _pad;
    float *out;
} tsm_slab_reduce;
/* dh2 / h1 / w2_slabs_out (nullable triple): the SECOND layer's weight gradient as extra column blocks of the same launch,
 * dW2 = dH2^T H1 over the same row chunks, from the activations launch (A) published in minibatch order
 * (tsm_critic_rows_grad_ppo: h1_out, dh2_out): w2_slabs_out [n_chunks][128 x 128].  Launch (A) then keeps no W2 gradient --
 * a rank-32 update per 32-row tile stored as a 64 KB slab (17 MB per BASELINE configs[2] step) becomes 32 chunk slabs (2 MB). */
int tsm_critic_rows_dw1(const float *dh1, const float *obs_rows, int32_t in_dim, const int64_t *rows, int64_t first_row,
                        int64_t tm_T, int64_t tm_E, int64_t Mr, int32_t n_chunks, float *w1_slabs_out,
                        const float *dh2, const float *h1, float *w2_slabs_out,
                        const tsm_slab_reduce *side, int32_t n_side, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Latency-grade all-reduce of a small vector over peer-mapped memory  [SURVEY 8e: the 45 KB shared-policy gradient]
 * Replaces  torch.distributed.all_reduce(flat_grad) in front of Optimizer.step (algorithm_base.py:485-498) for env-sharded
 *           replicas on one node (the reference itself has no distributed path: utils/net/common.py:477-519).
 * One-shot write-to-peers over IPC-mapped fine-grained memory (every element one 8-byte store {value, call stamp}: no fences),
 * one launch per call, rank-ordered sum (bit-identical on every rank); csrc/p2p.hip has the protocol.  Setup: every rank tsm_p2p_create -> tsm_p2p_export -> the ranks exchange
 * the tsm_p2p_ipc_handle_bytes()-byte handles by any channel (the host binding uses the process group) -> tsm_p2p_import of
 * every peer -> tsm_p2p_handshake on every rank (one stamped word per peer each way, bounded spin, outside any capture); the
 * ranks then AGREE (over their process group) to use this path only if every rank's handshake passed -- otherwise each destroys
 * its handle and the backend's own all-reduce serves for the rest of the process (the host binding: TSM_P2P_ALLREDUCE unset =
 * "the handshake decides", 1 = required, 0 = off).
 * Failure behaviour (fail-stop): a peer whose word does not arrive within the spin limit (tsm_p2p_set_timeout; ~2 s) sets the
 * handle's error word; the element that timed out is NOT updated (tsm_p2p_adam_step leaves parameter and moments as they
 * were, tsm_p2p_all_reduce leaves the element), every later launch on the handle is a no-op, and tsm_p2p_failed (synchronises
 * the device) returns 1: the host raises.  No hang, and no replica ever steps on a partial sum.
 * ------------------------------------------------------------------------------------------- */
int64_t tsm_p2p_ipc_handle_bytes(void);
int tsm_p2p_create(int32_t rank, int32_t world, int64_t max_floats, void **handle_out);
int tsm_p2p_export(void *handle, void *ipc_handle_out);
int tsm_p2p_import(void *handle, int32_t peer, const void *ipc_handle);
int tsm_p2p_all_reduce(void *handle, float *data, int64_t n, void *stream);
/* tsm_reduce_slabs (scale 1 / world) + tsm_p2p_all_reduce + tsm_adam_step (without a gradient-norm clip) in ONE launch: every
 * workgroup sums the slabs of its own slice of the parameter vector, runs the one-shot protocol on that slice and applies Adam to
 * it (the three steps have no grid-wide dependency), so the replicas' gradient step is one launch like the single-GPU step.
 * Bit-identical to the three-launch form.  Arguments as tsm_adam_step; n <= the handle's max_floats. */
int tsm_p2p_adam_step(void *handle, float *param, const float *grad_slabs, int32_t n_slab, int64_t n, float *exp_avg,
                      float *exp_avg_sq, int64_t step, const int64_t *step_dev, double lr, const double *lr_dev, double beta1,
                      double beta2, double eps, double weight_decay, float *param_image, const int32_t *image_map, void *stream);
int tsm_p2p_set_timeout(void *handle, double seconds);
int tsm_p2p_handshake(void *handle, int32_t *ok_out, void *stream);
TSM_VALUE int tsm_p2p_failed(void *handle);
/* The error word copied asynchronously into PINNED host memory behind the work queued on `stream`: valid once the host has waited
 * for that point of the stream.  The host binding queues it in front of the event of every update's loss statistics and raises
 * on every rank when it reads them (no extra synchronisation; algorithm/ppo.py, ppo_generic.py). */
int tsm_p2p_error_async(void *handle, int32_t *host_pinned_out, void *stream);
int tsm_p2p_destroy(void *handle);

/* ---------------------------------------------------------------------------------------------
 * CTDE global state  [a16]
 * Replaces  GlobalStateConstructor.build("concatenate" | "mean")
 *           (tianshou/algorithm/multiagent/ctde.py:291-300) for per-agent arrays [B][D] given in
 *           env.agents order (quirk Q5).  mode 0: out [B][N*D] concat; mode 1: out [B][D] mean.
 * With the joint-lane layout obs[..][N][D] the concatenation is a free reshape; this entry point
 * serves hosts that hold one array per agent (the reference's dict-of-tensors AoS).
 * ------------------------------------------------------------------------------------------- */
int tsm_global_state(const float *const *obs_by_agent_host, int32_t n_agent, int64_t B, int32_t D,
                     int mode, float *out, void *stream);

/* Minibatch permutations  [a14]
 * Replaces  the np.random.permutation(length) drawn by Batch.split(shuffle=True) once per repeat
 *           (tianshou/data/batch.py:1219 via ppo.py:179) when shuffling is done on the device.
 * Writes n_perm pseudo-random permutations of [0, n) in ONE launch (keyed Feistel network + cycle walking, key =
 * Philox(seed, counter + *counter_dev + p)):  out[p][i] = pi_p(i) * scale + (p / group_size) * offset_mul.
 * counter_dev (nullable, device u64[1]) lets a captured hipGraph draw fresh permutations on every replay
 * (advance it with tsm_u64_add). */
int tsm_random_permutations(int64_t n, int32_t n_perm, uint64_t seed, uint64_t counter, const uint64_t *counter_dev,
                            int64_t scale, int32_t group_size, int64_t offset_mul, int64_t *out, void *stream);
/* The same draw keyed by *counter_dev alone, after which the LAST workgroup to finish adds counter_inc to *counter_dev (every
 * workgroup has read it by then): a captured graph needs no tsm_u64_add launch behind its draws.  done_ctr: a zeroed u32 in HBM
 * owned by this call site (left at zero again). */
int tsm_random_permutations_advance(int64_t n, int32_t n_perm, uint64_t seed, uint64_t *counter_dev, uint64_t counter_inc,
                                    uint32_t *done_ctr, int64_t scale, int32_t group_size, int64_t offset_mul, int64_t *out,
                                    void *stream);

/* CTDEPolicy.learn loss head  [a16]
 * Replaces  the TD target / critic MSE / policy-gradient arithmetic of CTDEPolicy.learn
 *           (tianshou/algorithm/multiagent/ctde.py:149-185) between the network forwards and `backward()`.
 * q, q_next [B][n_out]: centralized critic on global_obs / global_obs_next (mean over n_out = the value, :154-157);
 * logits [B][n_act]: decentralized actor on the local obs; act i64 [B].  The (B,) x (B,1) broadcast of :185 is kept
 * (actor_loss = -mean(log_probs) * mean(advantage), quirk Q7).  Outputs: dq [B][n_out] = d critic_loss / d q,
 * dlogits [B][n_act] = d actor_loss / d logits, scalars[2] = {actor_loss, critic_loss}.
 * partial: tsm_ctde_head_partial_elems(B) doubles of scratch. */
int64_t tsm_ctde_head_partial_elems(int64_t B);
int tsm_ctde_td_head(const float *q, const float *q_next, int32_t n_out, const float *rew,
                     const uint8_t *terminated, float gamma, const float *logits, const int64_t *act,
                     int32_t n_act, int64_t B, float *dq, float *dlogits, double *partial, float *scalars,
                     void *stream);

/* ---------------------------------------------------------------------------------------------
 * Fully-connected networks of arbitrary width (f32 MFMA tiled GEMMs)  [a7, a16]
 * Replaces  nn.Linear / activation stacks and autograd through them for actor / critic modules that do not fit
 *           the fused 64-wide kernels: DecentralizedActor.forward (ctde.py:366-379), CentralizedCritic.forward
 *           (ctde.py:402-414), MLP (tianshou/utils/net/common.py:67-160), and `loss.backward()` (ctde.py:188-194).
 * params: flat f32 vector in torch `parameters()` order  w0[dims[1]][dims[0]], b0[dims[1]], w1, b1, ...
 * `act` (1 relu, 2 tanh, 0 none) follows every layer except the last.
 * tsm_mlp_forward : acts = consecutive blocks [B][dims[1]], [B][dims[2]], ... (the last block is the output);
 *                   tsm_mlp_act_elems(desc, B) floats.
 * tsm_mlp_backward: d_out [B][dims[L]] = gradient w.r.t. the output; writes n_split gradient slabs
 *                   slabs[n_split][n_param] (batch split; sum them with tsm_adam_step / tsm_reduce_slabs);
 *                   d_acts: workspace of tsm_mlp_act_elems floats (hidden-layer gradients).
 * ------------------------------------------------------------------------------------------- */
#define TSM_MLP_MAX_LAYERS 8
typedef struct tsm_mlp_desc {
    int32_t n_layers;
    int32_t act;
    int32_t dims[TSM_MLP_MAX_LAYERS + 1];
} tsm_mlp_desc;
int64_t tsm_mlp_param_count(const tsm_mlp_desc *desc);
int64_t tsm_mlp_act_elems(const tsm_mlp_desc *desc, int64_t B);
int tsm_mlp_forward(const tsm_mlp_desc *desc, const float *params, const float *x, int64_t B, float *acts,
                    void *stream);
/* tsm_mlp_forward whose launches are no-ops when *run_if_nonzero == 0 (device i32; read by every workgroup): lets a
 * captured graph hold a pass that is only needed for some inputs (see tsm_value_next_select). */
int tsm_mlp_forward_cond(const tsm_mlp_desc *desc, const float *params, const float *x, int64_t B, float *acts,
                         const int32_t *run_if_nonzero, void *stream);
int tsm_mlp_backward(const tsm_mlp_desc *desc, const float *params, const float *x, int64_t B, const float *acts,
                     const float *d_out, float *d_acts, int32_t n_split, float *slabs, int64_t slab_stride,
                     void *stream);
/* slab_stride: distance in floats between consecutive slabs (0 = this net's parameter count).  A larger stride lets
 * several networks write their gradients side by side into the slabs of ONE joint parameter vector (actor + critic
 * under one optimizer with a global gradient-norm clip, algorithm_base.py:485-498). */

/* ---------------------------------------------------------------------------------------------
 * QMIX  (tianshou/algorithm/multiagent/ctde.py:417-725)
 * tsm_qmix_mix_td replaces  QMIXMixer.forward on both sides + the TD target + mse_loss + the mixer's part of
 *           loss.backward() in QMIXPolicy.learn (ctde.py:468-499, 628-697), between the network forwards (tsm_mlp_forward)
 *           and the networks' backward (tsm_mlp_backward).  One launch over the B joint rows.
 *   agents:  per agent i < n_agents: q [B][n_act] (online Q-net on obs), q_next [B][n_act] (target Q-net on obs_next),
 *            act i64 [B], rew f32 [B]; out: dq [B][n_act] = d loss / d q, non-zero only at act.
 *   w1raw [B][n_agents * E], b1 [B][E], w2raw [B][E], b2 [B]: the online hypernetwork outputs on global_obs (hyper_w1,
 *            hyper_b1, hyper_w2, hyper_b2); tw1raw .. tb2 the target hypernetworks' on global_obs_next.  term u8 [B]: agent
 *            0's `terminated` (ctde.py:688).  monotonic != 0: w = |w_raw| (d|x|/dx = sign(x), sign(0) = 0).
 *   out: dw1 / db1 / dw2 / db2 = gradients w.r.t. the four online hypernetwork outputs (same layouts);
 *        partial f64 [tsm_qmix_partial_elems(B, E)] = per workgroup {sum (q_tot - y)^2, sum q_tot}.
 *        qtot_out (nullable) f32 [B]: q_tot of every row (QMIXMixer.forward alone: act = 0 with n_act = 1).
 *   Bounds: n_agents <= 8, E in {32, 64}, n_act <= 64; the [B][.] f32 arrays of the hypernetworks 16-byte aligned
 *   (TSM_ERR_INVALID otherwise).  No atomics: every output element has one writer.
 * tsm_qmix_finalize: out[2] = {loss = mse, q_values = mean(q_tot)} from the partials in a fixed order (one wave); out may
 *   be pinned host memory.
 * tsm_qmix_egreedy replaces  the epsilon-greedy choice of QMIXPolicy.forward (ctde.py:606-612) on the device:
 *   act_out[b * act_row_stride + i] = a uniform action in [0, n_act) when agent i's coin lands (u < *eps_dev), else the
 *   first argmax of q_i[b].  ONE coin per (call, agent), shared by the batch (quirk Q10).  Philox4x32-10 keyed by seed;
 *   counter c = offset + *offset_dev (offset_dev nullable): the coin of agent i is word 1 at c + i, the uniform action of
 *   (b, i) word 0 at c + b * n_agents + i -- a caller advancing c by B * n_agents per call keeps draws apart.
 *   act_row_stride >= n_agents (n_agents for the Collector's [E][N] action array).
 * ------------------------------------------------------------------------------------------- */
#define TSM_QMIX_MAX_AGENTS 8
typedef struct tsm_qmix_agents {
    const float *q[TSM_QMIX_MAX_AGENTS];
    const float *q_next[TSM_QMIX_MAX_AGENTS];
    const int64_t *act[TSM_QMIX_MAX_AGENTS];
    const float *rew[TSM_QMIX_MAX_AGENTS];
    float *dq[TSM_QMIX_MAX_AGENTS];
} tsm_qmix_agents;
int64_t tsm_qmix_partial_elems(int64_t B, int32_t E);
int tsm_qmix_mix_td(const tsm_qmix_agents *agents, int32_t n_agents, int32_t n_act, int64_t B, int32_t E,
                    const float *w1raw, const float *b1, const float *w2raw, const float *b2, const float *tw1raw,
                    const float *tb1, const float *tw2raw, const float *tb2, const uint8_t *term, float gamma,
                    int monotonic, float *dw1, float *db1, float *dw2, float *db2, double *partial, float *qtot_out,
                    void *stream);
int tsm_qmix_finalize(const double *partial, int32_t n_blocks, int64_t B, float *out, void *stream);
int tsm_qmix_egreedy(const float *const *q_by_agent_host, int32_t n_agents, int64_t B, int32_t n_act,
                     const float *eps_dev, uint64_t seed, uint64_t offset, const uint64_t *offset_dev, int32_t *act_out,
                     int64_t act_row_stride, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Gradient of a fully-connected net w.r.t. a window of its input
 * Replaces  the part of `actor_loss.backward()` that runs through critic_i back to agent i's action columns
 *           (MADDPGPolicy.learn, ctde.py:918-924).
 * tsm_mlp_input_grad: after tsm_mlp_forward(desc, params, x, B, acts): the dgrad chain of tsm_mlp_backward with NO
 *   weight-gradient launches, ended by dx[b][0 .. n_col) = dZ_0[b] . W_0[:, col0 .. col0 + n_col) (row pitch ldx floats).
 *   d_out [B][dims[L]]; d_acts: workspace of tsm_mlp_act_elems floats (n_layers > 1).  0 <= col0, col0 + n_col <= dims[0].
 * ------------------------------------------------------------------------------------------- */
int tsm_mlp_input_grad(const tsm_mlp_desc *desc, const float *params, const float *x, int64_t B, const float *acts,
                       const float *d_out, float *d_acts, int32_t col0, int32_t n_col, float *dx, int64_t ldx,
                       void *stream);

/* ---------------------------------------------------------------------------------------------
 * MADDPG  (tianshou/algorithm/multiagent/ctde.py:728-955)
 * Within one learn call the agents are independent (ctde.py:829-925 reads, for agent i, the batch, the target actors,
 * target critic i, critic i and actor i), so each entry serves all n_agents <= 8 agents in one launch.
 * tsm_maddpg_joint_rows replaces  the torch.cat chains that build the critics' inputs (ctde.py:875-880, 888, 893, 913-919).
 *   obs[i] [B][D], act[i] [B][Ad] (host arrays of device pointers).  W = n_agents * (D + Ad).
 *   replace == NULL: out [B][W], row b = [obs_0[b] .. obs_{N-1}[b] | act_0[b] .. act_{N-1}[b]].
 *   replace != NULL: out [n_agents][B][W]; matrix m is the same with replace[m][b] ([B][Ad]) in agent m's action slot.
 *   16-byte accesses for the regions whose rows allow them (D resp. Ad, their offsets and W multiples of 4, aligned
 *   pointers), scalar ones otherwise.
 * tsm_maddpg_td replaces  td_target, F.mse_loss and its gradient w.r.t. q (ctde.py:895-898) for every agent:
 *   y_i = rew_i + gamma q_next_i (1 - term_i) with agent i's OWN terminated flags, dq_i = 2 (q_i - y_i) / B, formed in f64
 *   from the f32 inputs and rounded once;
 *   partial f64 [tsm_maddpg_partial_elems(B, n_agents)] = per workgroup (256 rows) and agent the sum of (q_i - y_i)^2.
 *   No atomics: every output element has one writer.
 * tsm_maddpg_finalize replaces  the .item() reads of ctde.py:927-928: out[2 i] = actor_loss_i = -mean(q_pi[i]) with
 *   q_pi[i] [B] = critic_i on the rows carrying actor_i's action, out[2 i + 1] = critic_loss_i = the MSE from the
 *   partials; sums in f64 in a fixed order.  out f32 [2 n_agents] may be pinned host memory.
 * tsm_maddpg_act: the acting epilogue on the device (ctde.py:803-813 returns the actor output; exploration noise and the
 *   clamp to the Box are the caller's there): act_out [(e * n_agents + i)][k] = mu[i][e][k] + *sigma_dev * z, clamped to
 *   [low[k], high[k]] when the bounds are given (both or neither).  z: standard normal (Box-Muller on words 0 and 1 of
 *   Philox4x32-10 keyed by seed at counter offset + *offset_dev + element index).  *sigma_dev == 0 draws nothing and,
 *   without bounds, stores the actor's bits.
 * tsm_polyak replaces  update_target_networks (ctde.py:936-955): target[i] = tau * param[i] + (1 - tau) * target[i] with
 *   both products rounded to f32 before the sum (no FMA) and 1 - tau formed in double, then rounded to f32.
 * ------------------------------------------------------------------------------------------- */
#define TSM_MADDPG_MAX_AGENTS 8
typedef struct tsm_maddpg_agents {
    const float *q[TSM_MADDPG_MAX_AGENTS];
    const float *q_next[TSM_MADDPG_MAX_AGENTS];
    const float *rew[TSM_MADDPG_MAX_AGENTS];
    const uint8_t *term[TSM_MADDPG_MAX_AGENTS];
    float *dq[TSM_MADDPG_MAX_AGENTS];
} tsm_maddpg_agents;
int tsm_maddpg_joint_rows(const float *const *obs_by_agent_host, const float *const *act_by_agent_host,
                          const float *const *replace_by_agent_host, int32_t n_agents, int64_t B, int32_t D, int32_t Ad,
                          float *out, void *stream);
int64_t tsm_maddpg_partial_elems(int64_t B, int32_t n_agents);
int tsm_maddpg_td(const tsm_maddpg_agents *agents, int32_t n_agents, int64_t B, double gamma, double *partial,
                  void *stream);
int tsm_maddpg_finalize(const double *partial, int32_t n_blocks, const float *const *q_pi_by_agent_host,
                        int32_t n_agents, int64_t B, float *out, void *stream);
int tsm_maddpg_act(const float *const *mu_by_agent_host, int32_t n_agents, int64_t E, int32_t Ad, const float *sigma_dev,
                   uint64_t seed, uint64_t offset, const uint64_t *offset_dev, const float *low, const float *high,
                   float *act_out, void *stream);
int tsm_polyak(float *target, const float *param, int64_t n, double tau, void *stream);
/* tsm_adam_step (same arguments) with the coefficients 1 - beta1 and 1 - beta2 formed in f64 and rounded to f32 once, as
 * torch.optim.Adam forms them (`lerp_(grad, 1 - beta1)`, `addcmul_(grad, grad, value=1 - beta2)`).  tsm_adam_step and its kin
 * keep the f32 differences 1.f - (float)beta, bit for bit as before: 1.f - 0.999f lies 1.3e-5 below 0.001, which lengthens
 * every step by 6.4e-6 of itself along the gradient's sign.  MADDPG's actor loss is a MEAN over the outputs of the critic that
 * was just stepped, where that one-sided error does not average out, so its two optimizers use this entry. */
int tsm_adam_step_coef64(float *param, const float *grad_slabs, int32_t n_slab, int64_t n, float *exp_avg,
                         float *exp_avg_sq, int64_t step, const int64_t *step_dev, double lr, const double *lr_dev,
                         double beta1, double beta2, double eps, double weight_decay, double max_grad_norm, float *work,
                         float *param_image, const int32_t *image_map, void *stream);

/* ---------------------------------------------------------------------------------------------
 * n-step targets  (tianshou/algorithm/algorithm_base.py:720-815, 1155-1216)
 * tsm_nstep_return replaces  the `buffer.next` stack (:773-777), `value_mask` (:796), the end flags (:797-798) and the
 *           loop of `_nstep_return` (:1195-1211) of Algorithm.compute_nstep_return, for all I sampled flat indices in one
 *           launch (one thread per index, at most n_step dependent loads each).
 *   state / done_store: as for tsm_vrb_next.  term_store u8 [S][B][term_row_stride], column term_col.
 *   rew_store f32 [S][B][rew_row_stride], column rew_col: the agent's lane of a joint-step buffer, or the column that
 *   MARLDispatcher swaps in for `buffer.rew` on AEC rows (marl.py:231,240) -- the walk still visits ALL rows.
 *   out: idx_n i64 [I] = next^(n_step - 1)(indices); mc f32 [I] = the Monte-Carlo part; gpow f32 [I] = gamma^m with
 *        m = (first n with an end flag) + 1, else n_step; vmask u8 [I] = !terminated[idx_n].
 *        End flags are done | isin(index, unfinished_index()).  mc and gamma^m are float64 in registers, rounded once.
 *   returns = target_q(idx_n) * vmask * gpow + mc  is formed by the consumer (tsm_dqn_td_head).
 *   n_step < 1, gamma outside [0, 1], a column outside its row: TSM_ERR_INVALID.
 *
 * DQN  (tianshou/algorithm/modelfree/dqn.py)
 * tsm_dqn_check: the bounds of the DQN kernels (n_act in [1, 64], n_step >= 1; QLearningOffPolicyAlgorithm.__init__,
 *   dqn.py:235-237): TSM_ERR_INVALID naming the limit.
 * tsm_dqn_td_head replaces  DQN._target_q after its network forwards (dqn.py:365-379), `_nstep_return`'s last line
 *           (algorithm_base.py:1213-1215) and DQN._update_with_batch between `self.policy(batch).logits` and
 *           `optim.step(loss)` (dqn.py:387-402).  One launch over the B rows.
 *   q [B][n_act]: the online net on obs; q_next_online [B][n_act]: the online net on obs_next[idx_n]; q_next_target: the
 *   lagged net on the same rows, NULL when target_update_freq == 0 (the online values stand in).  mask_next u8 [B][n_act]
 *   (nullable): the action mask that travels with obs_next.  act i64 [B]; mc / gpow / vmask from tsm_nstep_return; weight
 *   f32 [B] (nullable: 1).  is_double != 0: target = q_target[first argmax of compute_q_value(q_next_online, mask)], else
 *   the row maximum of q_target.  compute_q_value's offset is min - max - 1 over the WHOLE q_next_online tensor
 *   (dqn.py:147-150): each workgroup reduces it itself.  huber_delta <= 0: loss = mean(td^2 weight); else
 *   huber_loss(q, returns, delta, "mean") (weight is not used, dqn.py:392-397).
 *   out: returns f32 [B]; td_error f32 [B] = returns - q[b][act[b]]; dq f32 [B][n_act] = d loss / d q, non-zero only at
 *        act; partial f64 [tsm_dqn_partial_elems(B)] = per workgroup {sum of loss terms, sum of q[b][act[b]]} -- the
 *        layout of tsm_qmix_mix_td's partials, so tsm_qmix_finalize(partial, n_blocks, B, out) gives
 *        out[2] = {loss, mean q[b][act[b]]} (out may be pinned host memory).
 * tsm_dqn_egreedy replaces  DiscreteQLearningPolicy.forward's argmax with add_exploration_noise (dqn.py:140-141, 153-171)
 *           on the device: q [R][n_act], mask u8 [R][n_act] (nullable).  Per row r: the first argmax of the masked q, or --
 *           when the ROW's coin lands (u < *eps_dev) -- the first argmax of uniform[n_act] + mask.  All draws of row r are
 *           words of Philox4x32-10 keyed by seed at counter offset + *offset_dev + r (offset_dev nullable), so a batch
 *           drawn in pieces with the offset advanced equals the batch drawn at once.  act_out i32 [R].
 * ------------------------------------------------------------------------------------------- */
#define TSM_DQN_ROWS_PER_BLOCK 256  /* one row per thread of the TD head (tsm_dqn_partial_elems counts by it) */
int tsm_nstep_return(const void *state, int64_t buffer_num, int64_t sub_size, const uint8_t *done_store,
                     const uint8_t *term_store, int64_t term_row_stride, int32_t term_col, const float *rew_store,
                     int64_t rew_row_stride, int32_t rew_col, const int64_t *indices, int64_t I, int32_t n_step,
                     double gamma, int64_t *idx_n, float *mc, float *gpow, uint8_t *vmask, void *stream);
int tsm_dqn_check(int32_t n_act, int32_t n_step);
int64_t tsm_dqn_partial_elems(int64_t B);
int tsm_dqn_td_head(const float *q, const float *q_next_online, const float *q_next_target, const uint8_t *mask_next,
                    const int64_t *act, const float *mc, const float *gpow, const uint8_t *vmask, const float *weight,
                    int64_t B, int32_t n_act, int is_double, float huber_delta, float *returns_out, float *td_error,
                    float *dq, double *partial, void *stream);
int tsm_dqn_egreedy(const float *q, const uint8_t *mask, int64_t R, int32_t n_act, const float *eps_dev, uint64_t seed,
                    uint64_t offset, const uint64_t *offset_dev, int32_t *act_out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Prioritized experience replay  (tianshou/data/utils/segtree.py, tianshou/data/buffer/prio.py)
 * The tree is the reference's: double tree[2 * bound], bound = tsm_segtree_bound(size) = the smallest power of two >= size
 * (-1 for a size outside [1, 2^30]); leaf i at tree[bound + i], node k = tree[2k] + tree[2k + 1], tree[1] the total,
 * padding leaves 0.  mark: i32 [bound] scratch of the set, all -1 before the first call and after every call.
 * err: one i64 word in HBM; a set / IS-weight launch that meets an index outside [0, size) skips that entry and stores 1
 * there -- tsm_segtree_check reads the word (one synchronisation), clears it and returns TSM_ERR_INVALID if it was set.
 * prio: f64 [2] = {max_prio, min_prio} in HBM, both 1.0 at the start (prio.py:39); read and folded on the device only.
 *
 * tsm_segtree_set replaces  `_setitem` (segtree.py:95-101) behind SegmentTree.__setitem__ (:35-51): leaves index[n] <-
 *           value[value_n], value_n == n or 1 (one value for all), then every ancestor.  One launch of one workgroup with a
 *           barrier per level.  Of several entries with one index the LAST wins, as in numpy's `tree[index] = value`.
 * tsm_segtree_prefix_sum_idx replaces  `_get_prefix_sum_idx` (segtree.py:119-134): per value[n] (f64) the descent from the
 *           root with `tree[left] < value` (strict) -> leaf indices i64 [n].  size == 1: 0.
 * tsm_segtree_reduce replaces  `_reduce` (segtree.py:104-116) behind SegmentTree.reduce(start, end) (:53-61): the sum of
 *           leaves [start, end) by the reference's additions in its order -> out f64 [1] in HBM.
 * tsm_per_sample replaces  `np.random.rand(batch_size) * self.weight.reduce()` + get_prefix_sum_idx of
 *           PrioritizedReplayBuffer.sample_indices (prio.py:63-66) in one launch: draw i = words 0, 1 of Philox4x32-10 at
 *           (seed, offset + *offset_dev + i) (offset_dev nullable), u = 52 bits * 2^-52, value = u * tree[1] < tree[1] for
 *           every draw (so no zero-weight padding leaf is reached) -> index_out i64 [n].
 * tsm_per_update_weight replaces  PrioritizedReplayBuffer.update_weight (prio.py:81-90): w = |td| + eps(f32) in float32,
 *           leaf = (double) w ** alpha with the power in float32 (alpha == 1: w itself), the set above, and
 *           prio <- {max(max_prio, max w), min(min_prio, min w)}.
 * tsm_per_init_weight replaces  init_weight (prio.py:46-47): leaves index[n] <- max_prio ** alpha, max_prio read from prio.
 * tsm_per_get_weight replaces  get_weight (prio.py:69-79) and the normalisation of __getitem__ (:103-106):
 *           (tree[bound + index] / min_prio) ** (-beta) in float64, divided by the batch maximum when weight_norm != 0
 *           -> out64 f64 [n] (the Batch the host API returns) and out32 f32 [n] = the same values rounded (the TD head's
 *           `weight`).  One workgroup.
 * ------------------------------------------------------------------------------------------- */
int64_t tsm_segtree_bound(int64_t size);
int tsm_segtree_set(double *tree, int32_t *mark, int64_t size, const int64_t *index, int64_t n, const double *value,
                    int64_t value_n, int64_t *err, void *stream);
int tsm_segtree_prefix_sum_idx(const double *tree, int64_t size, const double *value, int64_t n, int64_t *index_out,
                               void *stream);
int tsm_segtree_reduce(const double *tree, int64_t size, int64_t start, int64_t end, double *out, void *stream);
int tsm_segtree_check(int64_t *err, void *stream);
int tsm_per_sample(const double *tree, int64_t size, int64_t n, uint64_t seed, uint64_t offset, const uint64_t *offset_dev,
                   int64_t *index_out, void *stream);
int tsm_per_update_weight(double *tree, int32_t *mark, int64_t size, const int64_t *index, const float *td, int64_t n,
                          double alpha, double *prio, int64_t *err, void *stream);
int tsm_per_init_weight(double *tree, int32_t *mark, int64_t size, const int64_t *index, int64_t n, double alpha,
                        double *prio, int64_t *err, void *stream);
int tsm_per_get_weight(const double *tree, int64_t size, const int64_t *index, int64_t n, double beta, int weight_norm,
                       const double *prio, float *out32, double *out64, int64_t *err, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Distributional Q-learning: C51 and QR-DQN  (tianshou/algorithm/modelfree/c51.py, qrdqn.py; csrc/distq.hip)
 * The Q-network emits raw f32 [rows][n_act * n_atoms]; a row is read as [n_act][n_atoms].  The softmax over atoms that the
 * reference's Net(num_atoms=N, softmax=True) applies inside the module is part of these kernels.
 * tsm_distq_check: the bounds of the kernels (n_act in [1, 64] as for tsm_dqn_egreedy, n_atoms in [2, 256]; C51Policy.__init__,
 *   c51.py:56, QRDQN.__init__, qrdqn.py:78): TSM_ERR_INVALID naming the limit.
 * tsm_distq_values replaces  the reduction of C51Policy.compute_q_value (c51.py:67: `(logits * self.support).sum(2)`, with the
 *           module's softmax) when categorical != 0, of QRDQNPolicy.compute_q_value (qrdqn.py:20: `logits.mean(2)`) otherwise.
 *   raw [R][n_act][n_atoms]; support f32 [n_atoms] (categorical only: torch.linspace(v_min, v_max, n_atoms), filled by the
 *   host so that it holds the reference's values).  out: q f32 [R][n_act]; probs f32 [R][n_act][n_atoms] (nullable,
 *   categorical only): the softmax, `Batch.logits` of C51Policy.forward.  q feeds tsm_dqn_egreedy and the heads below.
 * tsm_c51_head replaces  C51._target_dist after its forwards (c51.py:123-141) and C51._update_with_batch between
 *           `self.policy(batch).logits` and `optim.step(loss)` (c51.py:150-158), with compute_nstep_return's last line for
 *           `_target_q` = the support (c51.py:120-121, algorithm_base.py:796, 1213-1215).  One launch.
 *   raw [B][n_act][n_atoms]: the online net on obs.  q_next [B][n_act]: tsm_distq_values of the ONLINE net on the successor
 *   rows; a* = its first argmax under mask_next (nullable) with compute_q_value's whole-tensor offset, as tsm_dqn_td_head.
 *   raw_next [B][n_act][n_atoms]: the lagged net on the same rows when there is one, else the online net's output.
 *   act i64 [B]; mc / gpow / vmask from tsm_nstep_return; weight f32 [B] (nullable: 1).
 *   returns[b][k] = (float)((double)(support[k] * vmask) * gpow + mc);  Tz = clamp(returns, v_min, v_max);
 *   m[j] = sum_k clamp(1 - |Tz[k] - support[j]| / dz, 0, 1) softmax(raw_next[b][a*])[k], dz = (v_max - v_min) / (n_atoms - 1);
 *   ce = -sum_j m[j] log(softmax(raw[b][act])[j] + 1e-8);  loss = mean(ce * weight).
 *   out: returns f32 [B][n_atoms]; prio f32 [B] = ce (`batch.weight` for a prioritized buffer); d_out f32 [B][n_act * n_atoms]
 *        = d loss / d raw through the 1e-8 and the softmax, zero off the taken action; partial f64
 *        [2 * ceil(B / TSM_DISTQ_ROWS_PER_BLOCK)] = per workgroup {sum ce * weight, sum E[z | act]} for tsm_qmix_finalize.
 * tsm_qrdqn_head replaces  QRDQN._target_q after its forwards (qrdqn.py:94-106), the same last line of the n-step return, and
 *           QRDQN._update_with_batch between `self.policy(batch).logits` and `optim.step(loss)` (qrdqn.py:113-129).  One launch.
 *   Arguments as above with raw values in place of logits; tau_hat f32 [n_quantiles]: the midpoints of
 *   torch.linspace(0, 1, n_quantiles + 1) (qrdqn.py:87-90), filled by the host.
 *   returns[b][j] = (float)((double)(raw_next[b][a*][j] * vmask) * gpow + mc);  u_ij = returns[j] - raw[b][act][i];
 *   loss_b = mean_i sum_j smooth_l1(u_ij) |tau_hat[i] - 1[u_ij <= 0]|;  loss = mean(loss_b * weight);
 *   prio[b] = mean_i sum_j |smooth_l1(u_ij)|;  the second partial is the mean quantile of the taken action.
 * Both heads: an action outside [0, n_act) reads nothing; the row's prio and loss term are NaN and its gradient zero.
 * ------------------------------------------------------------------------------------------- */
#define TSM_DISTQ_ROWS_PER_BLOCK 16
int tsm_distq_check(int32_t n_act, int32_t n_atoms);
int tsm_distq_values(const float *raw, const float *support, int64_t R, int32_t n_act, int32_t n_atoms, int categorical,
                     float *q, float *probs, void *stream);
int tsm_c51_head(const float *raw, const float *q_next, const float *raw_next, const uint8_t *mask_next, const int64_t *act,
                 const float *mc, const float *gpow, const uint8_t *vmask, const float *weight, const float *support,
                 int64_t B, int32_t n_act, int32_t n_atoms, double v_min, double v_max, float *returns_out, float *prio,
                 float *d_out, double *partial, void *stream);
int tsm_qrdqn_head(const float *raw, const float *q_next, const float *raw_next, const uint8_t *mask_next, const int64_t *act,
                   const float *mc, const float *gpow, const uint8_t *vmask, const float *weight, const float *tau_hat,
                   int64_t B, int32_t n_act, int32_t n_quantiles, float *returns_out, float *prio, float *d_out,
                   double *partial, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Discrete SAC  (tianshou/algorithm/modelfree/discrete_sac.py, sac.py `Alpha` / `AutoAlpha`; csrc/dsac.hip)
 * The actor emits logits f32 [B][n_act], each critic Q values f32 [B][n_act]; Categorical(logits) is part of these kernels:
 * ln = logits - logsumexp, p = softmax, H = -sum p ln (Categorical.entropy; its clamp of ln at finfo.min acts only at p = 0,
 * which finite logits never give), formed in float64 from the float32 logits and rounded where they leave.  alpha_dev f32 [1]
 * in HBM: the entropy coefficient, read on the device.
 * tsm_dsac_check: the bounds of the kernels (n_act in [1, 64] as for tsm_dqn_check, n_step >= 1): TSM_ERR_INVALID naming
 *   the limit.
 * tsm_dsac_target replaces  DiscreteSAC._target_q_compute_value (discrete_sac.py:147-155) after its forwards and
 *           `_nstep_return`'s last line (algorithm_base.py:796, 1213-1215).  One launch, one wave per row.
 *   logits_next: the ONLINE actor on obs_next[idx_n]; q1_next_old / q2_next_old: the two lagged critics on the same rows;
 *   mc / gpow / vmask from tsm_nstep_return.
 *   target_q = sum_a p[a] min(q1, q2)[a] + alpha H(p);  returns[b] = (float)((double)(target_q * vmask) * gpow + mc), the
 *   rounding rule of tsm_dqn_td_head.  out: returns f32 [B].
 * tsm_dsac_critic_head replaces  both critic losses of DiscreteSAC._update_with_batch (discrete_sac.py:162-174) between the
 *           critics' forwards and `critic_optim.step` / `critic2_optim.step`.  One launch.
 *   q1 / q2 [B][n_act]: the critics on obs; act i64 [B]; returns f32 [B]; weight f32 [B] (nullable: 1).
 *   td_i = q_i[b][act[b]] - returns[b]  (the reference's sign: the opposite of tsm_dqn_td_head's td_error).
 *   out: dq1 / dq2 f32 [B][n_act] = d mean(td_i^2 weight) / d q_i = 2 td_i weight / B at act, exactly zero elsewhere;
 *        prio f32 [B] = (td_1 + td_2) / 2 (`batch.weight` for a prioritized buffer, which takes the absolute value);
 *        partial f64 [2 * ceil(B / TSM_DSAC_ROWS_PER_BLOCK)] = per workgroup {sum td_1^2 weight, sum td_2^2 weight} in the
 *        layout of tsm_qmix_mix_td's partials: tsm_qmix_finalize gives out[2] = {critic1_loss, critic2_loss}.
 *   An action outside [0, n_act) reads nothing; the row's prio and loss terms are NaN and its gradient zero.
 * tsm_dsac_actor_head replaces  the actor loss of DiscreteSAC._update_with_batch and its backward down to the logits
 *           (discrete_sac.py:177-184), and the entropy that AutoAlpha.update reads (sac.py:203-205).  One launch.
 *   logits [B][n_act]: the actor on obs; q1 / q2 [B][n_act]: the critics on obs AFTER their own steps (constants here).
 *   loss_b = -(alpha H_b + sum_a p[a] min(q1, q2)[a]).
 *   out: entropy f32 [B]; d_logits f32 [B][n_act] = d mean_b(loss_b) / d logits
 *        = p[j] (alpha (ln[j] + H) - (q[j] - sum_a p[a] q[a])) / B;
 *        partial f64 (same size) = per workgroup {sum loss_b, sum H_b}: tsm_qmix_finalize gives {actor_loss, mean entropy}.
 * tsm_dsac_alpha_step replaces  AutoAlpha.update (sac.py:203-209) and the refresh of `alpha.value`: one launch of one wave
 *           on device scalars, no host read.
 *   entropy_partial f64 [2 * n_blocks]: tsm_dsac_actor_head's partials, of which the second of every pair is read; the mean
 *   entropy = their sum / B is formed in float64 in a fixed order and is not rounded to float32 before it is
 *   taken from target_entropy (near the target that difference is small against the entropy: one float32 ulp of the mean
 *   is several 1e-6 of it).  log_alpha, exp_avg, exp_avg_sq f32 [1], step i64 [1] (the count of steps taken so far;
 *   incremented here), all in HBM.
 *   alpha_loss = -(log_alpha * (target_entropy - mean entropy));  grad = -(target_entropy - mean entropy);  one torch Adam
 *   step (amsgrad off, 1 - beta formed in float64 as tsm_adam_step_coef64);  alpha_dev[0] = exp(log_alpha).
 *   out f32 [2] (HBM or mapped pinned memory) = {alpha_loss, the new alpha}.
 * ------------------------------------------------------------------------------------------- */
#define TSM_DSAC_ROWS_PER_BLOCK 16
int tsm_dsac_check(int32_t n_act, int32_t n_step);
int tsm_dsac_target(const float *logits_next, const float *q1_next_old, const float *q2_next_old, const float *alpha_dev,
                    const float *mc, const float *gpow, const uint8_t *vmask, int64_t B, int32_t n_act, float *returns_out,
                    void *stream);
int tsm_dsac_critic_head(const float *q1, const float *q2, const int64_t *act, const float *returns, const float *weight,
                         int64_t B, int32_t n_act, float *dq1, float *dq2, float *prio, double *partial, void *stream);
int tsm_dsac_actor_head(const float *logits, const float *q1, const float *q2, const float *alpha_dev, int64_t B,
                        int32_t n_act, float *entropy, float *d_logits, double *partial, void *stream);
int tsm_dsac_alpha_step(const double *entropy_partial, int32_t n_blocks, int64_t B, float *log_alpha, float *exp_avg,
                        float *exp_avg_sq, int64_t *step, double target_entropy, double lr, double beta1, double beta2,
                        double eps, double weight_decay, float *alpha_dev, float *out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Continuous-action actor-critics: DDPG, TD3, SAC  (tianshou/algorithm/modelfree/ddpg.py, td3.py, sac.py;
 * utils/net/continuous.py; csrc/cac.hip)
 * The actors emit raw (pre-tanh) outputs f32 [B][act_dim]; a critic reads rows [obs | act] of W = D + act_dim floats and emits
 * one Q value per row.  One launch each, one wave per row with action component k in lane k, no host reads; every stochastic
 * entry reads its standard normals from a buffer z f32 [B][act_dim] (tsm_cac_normal's, or a recorded draw).  Sums over the
 * action components are the xor butterfly in float64; loss sums leave as per-workgroup float64 pairs in tsm_qmix_mix_td's
 * layout, partial f64 [2 * ceil(B / TSM_CAC_ROWS_PER_BLOCK)], for tsm_qmix_finalize.  Two runs give the same bits.
 * tsm_cac_check: act_dim in [1, TSM_CAC_MAX_ACT_DIM], n_step >= 1: TSM_ERR_INVALID naming the limit.
 * tsm_cac_normal: z_out f32 [n] <- standard normals, Box-Muller on Philox(seed ^ a key of its own, offset + *offset_dev)
 *   with the block of four draws as third counter word (offset_dev nullable).
 * tsm_cac_det_action replaces  `max_action * tanh(.)` of ContinuousActorDeterministic.forward (continuous.py:86-88) and
 *           TD3's target smoothing (td3.py:196-199).
 *   rows_out[b * W + col0 + k] = max_action tanh(raw[b][k]) + clamp(policy_noise z[b][k], -noise_clip, noise_clip)
 *   (z nullable: no noise; noise_clip <= 0: no clamp; the sum is not clamped to the action bounds, as the reference).
 *   one_minus_tanh2_out f32 [B][act_dim] (nullable) <- 1 - tanh^2(raw), the backward's factor.
 * tsm_sac_action replaces  the epilogue of ContinuousActorProbabilistic.forward and SACPolicy.forward
 *           (continuous.py:238-247, sac.py:114-123).
 *   mu_raw[b * ld_mu + k], sigma_raw[b * ld_sigma + k] (ld_sigma = 0: one state-independent row);
 *   mu = max_action tanh(mu_raw) (unbounded != 0: mu_raw);  sigma = exp(clamp(sigma_raw, -20, 2));  x = mu + sigma z
 *   (z nullable: the mode);  a = tanh(x) -> rows_out[b * W + col0 + k];
 *   logp_out f32 [B] (nullable) = sum_k Normal(mu, sigma).log_prob(x) - sum_k log(1 - a^2 + finfo(float32).eps).
 * tsm_cac_target replaces  _target_q_compute_value (ddpg.py:314-325, td3.py:94-102, sac.py:298-302) after the forwards, and
 *           `_nstep_return`'s last line.  target_q = min(q1_next, q2_next) (q2_next nullable: q1_next) - alpha logp_next
 *   (logp_next nullable: nothing; each step rounded to float32);  returns_out f32 [B] by tsm_dqn_td_head's rounding rule.
 * tsm_cac_critic_head replaces  _minimize_critic_squared_loss (ddpg.py:267-285) between the forward and optimizer.step, for
 *           one critic (q2 null) or two.  td_i = q_i - returns in float64;  dq_i f32 [B] = 2 td_i weight / B (weight
 *   nullable: 1);  prio f32 [B] = td_1, or (td_1 + td_2) / 2;  partial = {sum td_1^2 weight, sum td_2^2 weight}.
 * tsm_cac_det_actor_head replaces  actor_loss = -critic(obs, actor(obs)).mean() and its backward down to the actor's raw
 *           output (ddpg.py:406, td3.py:216).  dq_da[b * ld + k] = d Q / d a (tsm_mlp_input_grad with d_out = 1);
 *   d_raw_out f32 [B][act_dim] = -dq_da max_action one_minus_tanh2 / B;  partial = {sum -q_pi, 0}.
 * tsm_sac_actor_head replaces  SAC's actor loss and its backward (sac.py:315-322) and the entropy AutoAlpha.update reads
 *           (:325).  mu_raw / sigma_raw / z as tsm_sac_action took them (the action terms are formed again from them);
 *   q1a, q2a f32 [B] (q2a nullable): the critics on [obs | a];  dq1_da, dq2_da [b * ld_g + k]: their input gradients with
 *   d_out = 1.  loss_b = alpha logp - min(q1a, q2a); the minimum's gradient goes to the smaller critic, half to each at a tie
 *   (torch.min's backward).  d_mu_out / d_sigma_out [b * ld_d + k] = d mean_b(loss_b) / d mu_raw, d sigma_raw (zero past the
 *   clamp; csrc/cac.hip derives the closed form);  logp_out f32 [B] (nullable);  partial = {sum loss_b, sum -logp}: the pair
 *   tsm_dsac_alpha_step reads.
 * tsm_cac_col_sum: the gradient of a state-independent sigma row (`sigma_param`, continuous.py:222) from the head's per-row
 *   d_sigma: slabs_out[k] = sum_b d[b * ld + k] (float64, fixed order), slabs_out[s * slab_stride + k] = 0 for the slabs
 *   1 <= s < n_slab (n_slab <= 64): the sigma columns of an actor's gradient slabs, ready for tsm_adam_step.
 * ------------------------------------------------------------------------------------------- */
#define TSM_CAC_MAX_ACT_DIM 64
#define TSM_CAC_ROWS_PER_BLOCK 16
int tsm_cac_check(int32_t act_dim, int32_t n_step);
int tsm_cac_normal(float *z_out, int64_t n, uint64_t seed, uint64_t offset, const uint64_t *offset_dev, void *stream);
int tsm_cac_det_action(const float *raw, const float *z, int64_t B, int32_t act_dim, double max_action, double policy_noise,
                       double noise_clip, float *rows_out, int64_t W, int32_t col0, float *one_minus_tanh2_out, void *stream);
int tsm_sac_action(const float *mu_raw, int64_t ld_mu, const float *sigma_raw, int64_t ld_sigma, const float *z, int64_t B,
                   int32_t act_dim, double max_action, int32_t unbounded, float *rows_out, int64_t W, int32_t col0,
                   float *logp_out, void *stream);
int tsm_cac_col_sum(const float *d, int64_t ld, int64_t B, int32_t act_dim, int32_t n_slab, float *slabs_out,
                    int64_t slab_stride, void *stream);
int tsm_cac_target(const float *q1_next, const float *q2_next, const float *logp_next, const float *alpha_dev,
                   const float *mc, const float *gpow, const uint8_t *vmask, int64_t B, float *returns_out, void *stream);
int tsm_cac_critic_head(const float *q1, const float *q2, const float *returns, const float *weight, int64_t B, float *dq1,
                        float *dq2, float *prio, double *partial, void *stream);
int tsm_cac_det_actor_head(const float *dq_da, int64_t ld, const float *one_minus_tanh2, const float *q_pi, int64_t B,
                           int32_t act_dim, double max_action, float *d_raw_out, double *partial, void *stream);
int tsm_sac_actor_head(const float *mu_raw, int64_t ld_mu, const float *sigma_raw, int64_t ld_sigma, const float *z,
                       const float *q1a, const float *q2a, const float *dq1_da, const float *dq2_da, int64_t ld_g,
                       const float *alpha_dev, int64_t B, int32_t act_dim, double max_action, int32_t unbounded,
                       float *d_mu_out, float *d_sigma_out, int64_t ld_d, float *logp_out, double *partial, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Offline continuous learners: CQL / Cal-QL and TD3+BC  (tianshou/algorithm/imitation/cql.py, td3_bc.py; csrc/cql.hip)
 * What the two updates add to the entries above.  With B transitions, R = num_repeat_actions, D = obs_dim, Ad = act_dim, a
 * flat index i in [0, B R) belongs to transition i / R.  All entries take a stream and read nothing from the host.
 * tsm_cql_check: act_dim in [1, TSM_CAC_MAX_ACT_DIM], num_repeat >= 1: TSM_ERR_INVALID naming the limit.  Needs no device.
 * tsm_cql_uniform replaces  torch.FloatTensor(B R, Ad).uniform_(-min_action, max_action) (cql.py:303-307).
 *   out f32 [n]: element e = lo + u01(word e % 4) (hi - lo), each step rounded to float32, of Philox4x32-10 under the key
 *   seed ^ a constant of its own at the ONE counter offset + *offset_dev (nullable) with e / 4 as third counter word -- the
 *   shape of tsm_cac_normal.  The caller advances its counter by n.  lo == hi gives lo everywhere (quirk Q70: the reference's
 *   defaults draw from uniform_(1, 1)).
 * tsm_cql_rows replaces  the repeat/view of obs and obs_next (cql.py:309-313) and the torch.cat([obs, act]) of the critic on
 *           the data rows and in _calc_random_values / _calc_pi_values (cql.py:218-241, 295-296).  One launch.
 *   obs, obs_next [B][D]; act [B][Ad]; rand_act [B R][Ad].
 *   x_out f32 [B + 3 B R][D + Ad]: rows [0, B) = [obs | act]; row B + i = [obs[i / R] | rand_act[i]]; rows B + B R + i and
 *   B + 2 B R + i = [obs[i / R] | untouched]: their action columns are tsm_sac_action's to fill (rows_out = row B + B R, col0 = D)
 *   from the actor on actor_rows_out.  The third group's action is sampled at obs_next but its row carries obs
 *   (`_calc_pi_values(tmp_obs_next, tmp_obs)`).
 *   actor_rows_out f32 [2 B R][D]: row i = obs[i / R], row B R + i = obs_next[i / R].
 * tsm_cql_head replaces  F.mse_loss, the calibration torch.max, torch.cat + torch.logsumexp, the Lagrange scaling and the
 *           backward of critic1_loss / critic2_loss down to the critics' outputs (cql.py:299-300, 331-384).  One launch for
 *           both critics, one thread per flat index, TSM_CQL_ROWS_PER_BLOCK of them per workgroup.
 *   q1, q2 f32 [B + 3 B R]: the critics on x_out; target [B]; logp_cur, logp_next [B R]: tsm_sac_action's logp of the second
 *   and third group; calib [B] (nullable: not calibrated); log_half_pow = log(0.5 ** Ad), formed by the host in float64;
 *   log_alpha f32 [1] in HBM (nullable: with_lagrange = False, cql_alpha = 1), read BEFORE tsm_cql_finalize steps it (Q72).
 *   csrc/cql.hip states the loss and its closed-form gradient; dq1, dq2 f32 [B + 3 B R] <- d loss_k / d q_k, every entry
 *   written; partial f64 [6 * ceil(B R / TSM_CQL_ROWS_PER_BLOCK)] = per workgroup and critic {sum (q - target)^2, sum q[b],
 *   sum lse_i}.
 * tsm_cql_finalize replaces  the scalars of cql.py:353-384 and cql_alpha_loss.backward() + cql_alpha_optim.step().  One launch
 *           of one thread, the workgroups' partials in index order.
 *   out f32 [6] (HBM or mapped pinned memory) = {critic1_loss, critic2_loss, cql_alpha, cql_alpha_loss = -(cql_1 + cql_2) / 2,
 *   d cql_alpha_loss / d log_alpha (zero where the clamp is active), log_alpha after the step}; the last four NaN with
 *   log_alpha null.  exp_avg, exp_avg_sq f32 [1] and step i64 [1] in HBM (null together: log_alpha is not stepped): one
 *   torch Adam step on log_alpha with that gradient (amsgrad off, no weight decay, 1 - beta formed in float64).
 * tsm_td3bc_actor_head replaces  TD3+BC's actor loss and its backward down to the actor's raw output (td3_bc.py:113-119).
 *           TWO launches: one workgroup sums {|q_pi|, q_pi} over the batch in a fixed order into qsum_work f64 [2] (the
 *           gradient of every row depends on mean |q_pi|), then the head reads that device scalar.
 *   dq_da[b * ld + k] = d Q / d a (tsm_mlp_input_grad with d_out = 1); one_minus_tanh2 [B][Ad] (tsm_cac_det_action's);
 *   q_pi [B]; act_pi[b * ld_a + k]: the policy's action (the action columns of the critic's rows); act_data [B][Ad].
 *   lmbda = alpha / mean |q_pi| (a constant of the backward);  actor_loss = -lmbda mean(q_pi) + mean((a - a_data)^2);
 *   d_raw_out f32 [B][Ad] = (-lmbda / B dq_da + 2 (a - a_data) / (B Ad)) max_action one_minus_tanh2;
 *   partial f64 [2 * ceil(B / TSM_CAC_ROWS_PER_BLOCK)] = {sum_b (-lmbda q_pi[b] + sum_k (a - a_data)^2 / Ad), 0}:
 *   tsm_qmix_finalize(partial, n_blocks, B, out) gives {actor_loss, 0}.
 * ------------------------------------------------------------------------------------------- */
#define TSM_CQL_ROWS_PER_BLOCK 256
int tsm_cql_check(int32_t act_dim, int32_t num_repeat);
int tsm_cql_uniform(float *out, int64_t n, double lo, double hi, uint64_t seed, uint64_t offset, const uint64_t *offset_dev,
                    void *stream);
int tsm_cql_rows(const float *obs, const float *obs_next, const float *act, const float *rand_act, int64_t B,
                 int32_t num_repeat, int32_t obs_dim, int32_t act_dim, float *x_out, float *actor_rows_out, void *stream);
int tsm_cql_head(const float *q1, const float *q2, const float *target, const float *logp_cur, const float *logp_next,
                 const float *calib, int64_t B, int32_t num_repeat, double log_half_pow, double temperature, double cql_weight,
                 double alpha_min, double alpha_max, const float *log_alpha, float *dq1, float *dq2, double *partial,
                 void *stream);
int tsm_cql_finalize(const double *partial, int64_t n_blocks, int64_t B, int32_t num_repeat, double cql_weight,
                     double lagrange_threshold, double alpha_min, double alpha_max, float *log_alpha, float *exp_avg,
                     float *exp_avg_sq, int64_t *step, double lr, double beta1, double beta2, double eps, float *out,
                     void *stream);
int tsm_td3bc_actor_head(const float *dq_da, int64_t ld, const float *one_minus_tanh2, const float *q_pi, const float *act_pi,
                         int64_t ld_a, const float *act_data, int64_t B, int32_t act_dim, double max_action, double alpha,
                         double *qsum_work, float *d_raw_out, double *partial, void *stream);

/* ---------------------------------------------------------------------------------------------
 * BCQ: VAE action model, perturbation actor, target and acting  (tianshou/algorithm/imitation/bcq.py;
 * utils/net/continuous.py:395-513; csrc/bcq.hip)
 * With B transitions, K = num_sampled_action, S = forward_sampled_times, L = latent_dim, D = obs_dim, Ad = act_dim.  The encoder
 * emits head f32 [B][2 L] = [mean | raw log_std]; the decoder reads rows [obs | z] of D + L floats and emits raw (pre-tanh)
 * actions; the perturbation net and the critics read rows [obs | act] of D + Ad floats.  All entries take a stream and read
 * nothing from the host; all are row-wise, float64 arithmetic from the float32 inputs rounded once; every documented output
 * element is written and no other; rows need no alignment.  The normals are tsm_cac_normal's.
 * tsm_bcq_check: act_dim in [1, TSM_CAC_MAX_ACT_DIM], latent_dim in [1, 2 TSM_CAC_MAX_ACT_DIM], num_sampled >= 1:
 *   TSM_ERR_INVALID naming the limit.  Needs no device.
 * tsm_bcq_latent replaces  the clamp, exp and reparameterised latent of VAE.forward and the torch.cat([state, z]) of decode
 *           (continuous.py:487-495, 513).  std_out f32 [B][L] = exp(clamp(head[b][L + j], -4, 15));
 *   x_dec_out f32 [B][D + L] = [obs[b] | head[b][j] + std eps[b][j]].
 * tsm_bcq_decode_rows replaces  repeat_interleave (bcq.py:213), the clamp of decode's normals (continuous.py:508-510) and its
 *           torch.cat, for two groups of observations in one launch.  src_a [n_a][D] with each row repeated rep_a times,
 *   src_b [n_b][D] (n_b = 0: src_b nullable), z [n_a rep_a + n_b][L] unclamped normals.
 *   rows_out f32 [n_a rep_a + n_b][D + L]: row i < n_a rep_a = [src_a[i / rep_a] | clamp(z[i], -0.5, 0.5)], row n_a rep_a + j =
 *   [src_b[j] | clamp(z[n_a rep_a + j], -0.5, 0.5)]; a NaN normal stays a NaN.
 * tsm_bcq_action_rows replaces  max_action * tanh(decoder(.)) (continuous.py:513) and the torch.cat([obs, act]) behind it.
 *   raw [n][Ad], x_dec [n][D + L];  x_out f32 [n][D + Ad] = [x_dec[i][:D] | max_action tanh(raw[i])].
 * tsm_bcq_target replaces  bcq.py:223-237.  q1, q2 f32 [B K]: the LAGGED critics on the K decoded (not perturbed) actions of
 *           every obs_next; rew [B]; vmask u8 [B] = not done.
 *   target_out f32 [B] = rew + vmask f32(gamma) max_k(lmbda min(q1, q2) + (1 - lmbda) max(q1, q2)); a NaN is kept.
 * tsm_bcq_vae_head replaces  recon_loss, KL_loss (bcq.py:203-206) and the backward of vae_loss down to the decoder's raw
 *           output.  raw_dec [B][Ad], act [B][Ad], head [B][2 L].  csrc/cac.hip's shape: TSM_CAC_ROWS_PER_BLOCK rows per
 *           workgroup of four waves, each wave walking four rows one after another, a row's components across its lanes.
 *   d_raw_out f32 [B][Ad] = 2 (recon - act) / (B Ad) max_action (1 - tanh^2(raw_dec)), recon = max_action tanh(raw_dec);
 *   partial f64 [2 * ceil(B / TSM_CAC_ROWS_PER_BLOCK)] = {sum_b (sum_k (act - recon)^2 / Ad + kl_b / (2 L)), sum_b kl_b / L},
 *   kl_b = sum_j (-clamp(ls) + (std^2 + mean^2 - 1) / 2):  tsm_qmix_finalize(partial, n_blocks, B, out) gives
 *   {vae_loss = recon_loss + KL_loss / 2, KL_loss}.  (The sums are scaled per row, not the raw {sum (act - recon)^2, sum kl}, so that
 *   the existing finalize's division by B is all that is left and no BCQ finalize is needed.)
 * tsm_bcq_latent_grad: the decoder's input gradient -> the gradient of the encoder's output.  dz [B][L]: tsm_mlp_input_grad of
 *           the decoder on columns [D, D + L) with d_out = d_raw_out;  head, eps as tsm_bcq_latent took them.
 *   d_head_out f32 [B][2 L]: [b][j] = dz + mean / (2 B L);  [b][L + j] = m (dz eps std + (std^2 - 1) / (2 B L)) with m = 1 where
 *   -4 <= ls <= 15 (torch.clamp's backward: bounds included), else 0.
 * tsm_bcq_perturb replaces  Perturbation.forward behind its net (continuous.py:429-432).  raw_p [n][Ad]: the net on x_in
 *           [n][D + Ad], whose action columns hold the base action a.  With u = a + phi max_action tanh(raw_p):
 *   x_out f32 [n][D + Ad] (not x_in) = [x_in[i][:D] | clamp(u, -max_action, max_action)];
 *   factor_out f32 [n][Ad] (nullable) = phi (1 - tanh^2(raw_p)) where -max_action <= u <= max_action, else 0: with
 *   tsm_cac_det_actor_head(dq_da, factor, q_pi, max_action) the actor's loss -mean Q and its gradient at raw_p.
 * tsm_bcq_select replaces  q1.argmax(0) and act[max_indice] per observation (bcq.py:103-115).  q f32 [n S]; the candidate
 *           actions rows[(g S + s) * ld + col0 + k].  One wave per observation.
 *   index_out i32 [n] = the FIRST s with the maximal q of group g (a NaN counts as the maximum, as torch.argmax);
 *   act_out f32 [n][Ad] = that candidate's action, bit for bit.
 * ------------------------------------------------------------------------------------------- */
int tsm_bcq_check(int32_t act_dim, int32_t latent_dim, int32_t num_sampled);
int tsm_bcq_latent(const float *head, const float *eps, const float *obs, int64_t B, int32_t obs_dim, int32_t latent_dim,
                   float *x_dec_out, float *std_out, void *stream);
int tsm_bcq_decode_rows(const float *src_a, int64_t n_a, int32_t rep_a, const float *src_b, int64_t n_b, const float *z,
                        int32_t obs_dim, int32_t latent_dim, float *rows_out, void *stream);
int tsm_bcq_action_rows(const float *raw, const float *x_dec, int64_t n, int32_t obs_dim, int32_t latent_dim, int32_t act_dim,
                        double max_action, float *x_out, void *stream);
int tsm_bcq_target(const float *q1, const float *q2, const float *rew, const uint8_t *vmask, int64_t B, int32_t num_sampled,
                   double gamma, double lmbda, float *target_out, void *stream);
int tsm_bcq_vae_head(const float *raw_dec, const float *act, const float *head, int64_t B, int32_t act_dim, int32_t latent_dim,
                     double max_action, float *d_raw_out, double *partial, void *stream);
int tsm_bcq_latent_grad(const float *dz, const float *head, const float *eps, int64_t B, int32_t latent_dim, float *d_head_out,
                        void *stream);
int tsm_bcq_perturb(const float *raw_p, const float *x_in, int64_t n, int32_t obs_dim, int32_t act_dim, double phi,
                    double max_action, float *x_out, float *factor_out, void *stream);
int tsm_bcq_select(const float *q, const float *rows, int64_t ld, int32_t col0, int64_t n, int32_t num_sampled, int32_t act_dim,
                   float *act_out, int32_t *index_out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Implicit Quantile Network (tianshou/algorithm/modelfree/iqn.py; utils/net/discrete.py:127-217; csrc/iqn.hip)
 * A network row is (b, s) = b * sample_size + s: out f32 [R][sample_size][n_act] (the reference's [B, A, S] logits are its
 * transposed view), e / phi f32 [R * sample_size][embedding_dim], taus f32 [R][sample_size].  The MLPs before and after the
 * embedding run through tsm_mlp_forward / tsm_mlp_backward / tsm_mlp_input_grad.
 * tsm_iqn_check: the bounds of the kernels (num_cosines a multiple of 4 in [4, 64], embedding_dim a multiple of 16 in
 *   [16, 512], sample_size in [2, 64], n_act in [1, 64]): TSM_ERR_INVALID naming the limit.  Needs no device.
 * tsm_iqn_taus replaces  `torch.rand(batch_size, sample_size)` of ImplicitQuantileNetwork.forward (discrete.py:211).
 *   Row r draws at Philox4x32-10 counter offset + *offset_dev (nullable) + r, as tsm_dqn_egreedy counts its rows, under a
 *   key that differs from that of the epsilon draws, so a policy may hand both the same counter.  Values in [0, 1).
 * tsm_iqn_embed_forward replaces  CosineEmbeddingNetwork.forward and the product `logits.unsqueeze(1) * embed(taus)`
 *           (discrete.py:145-161, 212-215).  One launch; the cosines never reach HBM.
 *   f [R][embedding_dim]: the preprocess net's last LINEAR output; relu_f != 0 applies the ReLU with which the reference's
 *   Net ends (common.py: every hidden layer is followed by its activation) here, g = relu, else g = identity.
 *   We [embedding_dim][num_cosines], be [embedding_dim].
 *   c[i] = cosf(tau * (f32(pi) * f32(i))), i = 1 .. num_cosines, each product rounded to f32;  phi = relu(We c + be) on f32
 *   MFMA;  e[b,s] = g(f[b]) * phi[b,s].  out: e, and phi for the backward.
 * tsm_iqn_embed_backward replaces  `loss.backward()` through the same lines.  One launch.
 *   d_e [R * sample_size][embedding_dim]: the gradient at `last`'s input (tsm_mlp_input_grad).
 *   out: d_f[b] = g'(f[b]) sum_s d_e[b,s] * phi[b,s] (s in order) for tsm_mlp_backward of the preprocess net; into slab z of n_split
 *   (the batch rows ceil(R / n_split) z ..., all their samples): dWe at w_off = (d_e * g(f) * 1[phi > 0])^T c on f32 MFMA with
 *   the cosines formed again, dbe at b_off its column sums.  Every slab is written in full.
 * tsm_iqn_values replaces  QRDQNPolicy.compute_q_value's `logits.mean(2)` (qrdqn.py:20) on out [R][sample_size][n_act]:
 *   q f32 [R][n_act], the sum over s in order / sample_size.  q feeds tsm_dqn_egreedy and tsm_iqn_head.
 * tsm_iqn_head replaces  QRDQN._target_q after its forwards (qrdqn.py:94-106), `_nstep_return`'s last line
 *           (algorithm_base.py:796, 1213-1215) and IQN._update_with_batch between `self.policy(batch)` and
 *           `optim.step(loss)` (iqn.py:160-181).  One launch.
 *   out [B][n_online][n_act]: the online net on obs, drawn with taus [B][n_online].  q_next [B][n_act]: tsm_iqn_values of the
 *   ONLINE net on the successor rows; a* = its first argmax under mask_next (nullable), as tsm_dqn_td_head.
 *   out_next [B][n_target][n_act]: the lagged net there, or that same online forward when there is no lagged net.
 *   returns[b][j] = (float)((double)(out_next[b][j][a*] * vmask) * gpow + mc);  u_ij = returns[j] - out[b][i][act];
 *   loss_b = (1 / n_online) sum_i sum_j smooth_l1(u_ij) |taus[b][i] - 1[u_ij <= 0]|;  loss = mean(loss_b * weight);
 *   prio[b] = (1 / n_online) sum_i sum_j |smooth_l1(u_ij)|.
 *   out: returns f32 [B][n_target]; prio f32 [B]; d_out f32 [B][n_online][n_act], exactly zero off the taken action; partial
 *        f64 [2 * ceil(B / TSM_IQN_ROWS_PER_BLOCK)] = per workgroup {sum loss_b weight, sum mean_i out[b][i][act]} for
 *        tsm_qmix_finalize.  An action outside [0, n_act) reads nothing: the row's loss, prio and q are NaN, its gradient zero.
 * ------------------------------------------------------------------------------------------- */
#define TSM_IQN_ROWS_PER_BLOCK 16
int tsm_iqn_check(int32_t num_cosines, int32_t embedding_dim, int32_t sample_size, int32_t n_act);
int tsm_iqn_taus(int64_t R, int32_t sample_size, uint64_t seed, uint64_t offset, const uint64_t *offset_dev, float *taus,
                 void *stream);
int tsm_iqn_embed_forward(const float *f, const float *taus, const float *We, const float *be, int64_t R,
                          int32_t sample_size, int32_t num_cosines, int32_t embedding_dim, int relu_f, float *e, float *phi,
                          void *stream);
int tsm_iqn_embed_backward(const float *d_e, const float *f, const float *phi, const float *taus, int64_t R,
                           int32_t sample_size, int32_t num_cosines, int32_t embedding_dim, int relu_f, float *d_f, int32_t n_split,
                           float *slabs, int64_t slab_stride, int64_t w_off, int64_t b_off, void *stream);
int tsm_iqn_values(const float *out, int64_t R, int32_t sample_size, int32_t n_act, float *q, void *stream);
int tsm_iqn_head(const float *out, const float *q_next, const float *out_next, const uint8_t *mask_next, const float *taus,
                 const int64_t *act, const float *mc, const float *gpow, const uint8_t *vmask, const float *weight, int64_t B,
                 int32_t n_act, int32_t n_online, int32_t n_target, float *returns_out, float *prio, float *d_out,
                 double *partial, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Fully parameterized Quantile Function  (tianshou/algorithm/modelfree/fqf.py; utils/net/discrete.py:220-315; csrc/fqf.hip)
 * Conventions of the IQN block: a network row is (b, i) = b * num_fractions + i, out f32 [R][num_fractions][n_act]; f [R]
 * [embedding_dim] is the preprocess net's last LINEAR output and relu_f != 0 applies its ReLU inside the kernel.  The embedding
 * at the proposed fractions is tsm_iqn_embed_forward / _backward.  Arithmetic is f32 unless said otherwise.
 * tsm_fqf_check: the bounds of the kernels (num_fractions in [3, 64] -- the interior forward has num_fractions - 1 fractions,
 *   the embedding takes 2 .. 64 --, embedding_dim a multiple of 16 in [16, 512], n_act in [1, 64]): TSM_ERR_INVALID naming the
 *   limit.  Needs no device.
 * tsm_fqf_propose replaces  FractionProposalNetwork.forward (discrete.py:240-253).  One launch.
 *   Wf [num_fractions][embedding_dim], bf [num_fractions].  logits = Wf g(f) + bf on f32 MFMA (k = 0 .. embedding_dim - 1 in
 *   order, then the bias), f32.  From there on the row is carried in float64 and every output rounded to f32 once (as
 *   tsm_dsac_* form their probabilities): e[n] = exp(x[n] - max x), se = sum_k e[k] (k in order), p[n] = e[n] / se,
 *   logp[n] = (x[n] - max x) - log(se);  taus[0] = 0, taus[k + 1] = taus[k] + p[k], k in order (taus[num_fractions] is what
 *   the sum gives, not forced to 1);  tau_hats[i] = (taus[i] + taus[i + 1]) / 2;  entropies = -(sum_n p[n] logp[n]), n in order.
 *   out: taus [R][num_fractions + 1], tau_hats [R][num_fractions], logp [R][num_fractions] (for the head), entropies [R].
 *   The features are detached (discrete.py:305): there is no d_f.
 * tsm_fqf_propose_backward replaces  `fraction_optim.step(...)`'s backward through the same lines.  One launch.
 *   d_logits [R][num_fractions] (tsm_fqf_head).  Into slab z of n_split (the rows ceil(R / n_split) z ..., the partition of
 *   tsm_iqn_embed_backward): dWf at w_off = d_logits^T g(f) on f32 MFMA, four rows per step in row order; dbf at b_off its column
 *   sums.  Every slab is written in full, an empty one as zeros.
 * tsm_fqf_values replaces  `((taus[:, 1:] - taus[:, :-1]).unsqueeze(1) * logits).sum(2)` of FQFPolicy.forward (fqf.py:94-97):
 *   q[r][a] = sum_i (taus[r][i + 1] - taus[r][i]) * out[r][i][a], i in order, each product rounded (no fma).  q feeds
 *   tsm_dqn_egreedy and tsm_fqf_head.
 * tsm_fqf_head replaces  FQF._target_q after its forwards (fqf.py:178-193), `_nstep_return`'s last line
 *           (algorithm_base.py:796, 1213-1215) and FQF._update_with_batch between `self.policy(batch)` and the two optimizer
 *           steps (fqf.py:201-247).  One launch.
 *   out [B][N][n_act]: the online net on obs at tau_hats;  out_tau [B][N - 1][n_act]: the same net at taus[:, 1:-1];
 *   q_next [B][n_act]: tsm_fqf_values of the ONLINE net on the successor rows;  out_next [B][N][n_act]: the lagged net there
 *   at the online proposal's tau_hats, or that same online forward when there is no lagged net.
 *   Quantile part: returns, loss, prio and d_out are tsm_iqn_head's with n_online = n_target = N and fraction tau_hats[b][i],
 *   in its rounding order; d_out is exactly zero off the taken action.
 *   Fraction part (fqf.py:227-243), Qh_i = out[b][i][act], Q_i = out_tau[b][i][act], i = 0 .. N - 2:
 *     v1 = Q_i - Qh_i, s1 = Q_i > (i == 0 ? Qh_0 : Q_{i-1});  v2 = Q_i - Qh_{i+1}, s2 = Q_i < (i == N - 2 ? Qh_{N-1} : Q_{i+1});
 *     g_{i+1} = (s1 ? v1 : -v1) + (s2 ? v2 : -v2);  with p = expf(logp) and taus [B][N + 1] as tsm_fqf_propose wrote them
 *     (the fractions at which out_tau was evaluated):
 *     fraction_loss_b = sum_k g_k taus_k (xor butterfly over the lanes);  G_m = g_{N-1} + g_{N-2} + ... + g_{m+1} in that order;
 *     Gbar = sum_n p_n G_n (butterfly);  d_logits[b][m] = (p_m (G_m - Gbar) + ent_coef * (p_m (logp_m + entropies[b]))) / B:
 *     the gradient of mean_b fraction_loss_b - ent_coef * mean_b entropies[b] with respect to the fraction layer's logits.
 *     The importance weight does not enter the fraction part.
 *   out: returns f32 [B][N]; prio f32 [B]; d_out f32 [B][N][n_act]; d_logits f32 [B][N]; partial and partial_frac f64
 *        [2 * ceil(B / TSM_IQN_ROWS_PER_BLOCK)] each = per workgroup {sum loss_b weight, sum mean_i Qh_i} and {sum
 *        fraction_loss_b, sum entropies[b]}, each for tsm_qmix_finalize.  An action outside [0, n_act) reads nothing: the
 *        row's quantile loss, prio, q and fraction loss are NaN, its d_out and d_logits rows zero.
 * ------------------------------------------------------------------------------------------- */
int tsm_fqf_check(int32_t num_fractions, int32_t embedding_dim, int32_t n_act);
int tsm_fqf_propose(const float *f, const float *Wf, const float *bf, int64_t R, int32_t num_fractions, int32_t embedding_dim,
                    int relu_f, float *taus, float *tau_hats, float *logp, float *entropies, void *stream);
int tsm_fqf_propose_backward(const float *d_logits, const float *f, int64_t R, int32_t num_fractions, int32_t embedding_dim,
                             int relu_f, int32_t n_split, float *slabs, int64_t slab_stride, int64_t w_off, int64_t b_off,
                             void *stream);
int tsm_fqf_values(const float *out, const float *taus, int64_t R, int32_t num_fractions, int32_t n_act, float *q,
                   void *stream);
int tsm_fqf_head(const float *out, const float *out_tau, const float *q_next, const float *out_next, const uint8_t *mask_next,
                 const float *taus, const float *tau_hats, const float *logp, const float *entropies, const int64_t *act, const float *mc,
                 const float *gpow, const uint8_t *vmask, const float *weight, double ent_coef, int64_t B, int32_t n_act,
                 int32_t num_fractions, float *returns_out, float *prio, float *d_out, float *d_logits, double *partial,
                 double *partial_frac, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Rainbow: NoisyLinear layers and dueling streams  (tianshou/algorithm/modelfree/rainbow.py; utils/net/discrete.py:318-375;
 * utils/net/common.py:319-364; csrc/rainbow.hip)
 * A net is ONE flat f32 vector [P] in the reference module's `parameters()` order, described by a table of its layers
 * (tsm_noisy_net, a HOST struct passed by pointer and handed to the kernels by value):
 *   noisy layer  mu_W [out][in] | sigma_W [out][in] | mu_bias [out] | sigma_bias [out] | eps_p [in] | eps_q [out]   at `off`
 *   plain layer  weight [out][in] | bias [out]                                                                      at `off`
 * and its EFFECTIVE vector [P_eff] holds W [out][in] | b [out] per layer at `eff_off`, the layout of tsm_mlp_* (trunk, then
 * the Q stream, then the V stream).  `slot_off` numbers the layer's noise slots (eps_p then eps_q) among all slots of the net.
 * All arithmetic is f32, every product rounded (no fma).
 * tsm_rainbow_check: the table's bounds (1 .. TSM_NOISY_MAX_LAYERS layers, in / out in [1, 65536], the three offsets of every
 *   layer exactly where the layers before it end, the totals P, P_eff and n_slots): TSM_ERR_INVALID naming the limit.  Every
 *   entry point below runs it first, so no kernel reads or writes outside [0, P) / [0, P_eff).  Needs no device.
 * tsm_noisy_sample replaces  NoisyLinear.sample / .f (discrete.py:358-365) for every noisy layer of a net.  One launch.
 *   Slot s gets sign(x) * sqrtf(|x|), x ~ N(0, 1): Philox block (seed ^ a key of this site's own, counter = offset +
 *   *offset_dev, sub = s / 4) gives words w0 .. w3; u1 = ((w >> 8) + 1) / 2^24 in (0, 1], u2 = (w >> 8) / 2^24;
 *   r = sqrtf(-2 logf(u1)); slots 4k, 4k + 1 = r cosf(2 pi u2), r sinf(2 pi u2) of (w0, w1), slots 4k + 2, 4k + 3 of (w2, w3).
 *   Only the distribution is the reference's (it draws with torch.randn), not the numbers.
 * tsm_noisy_compose replaces  the weight / bias lines of NoisyLinear.forward (discrete.py:368-373) for every layer.  One launch.
 *   training != 0: W[o][i] = mu_W[o][i] + sigma_W[o][i] * (eps_q[o] * eps_p[i]),  b[o] = mu_bias[o] + sigma_bias[o] * eps_q[o];
 *   training == 0: W = mu_W, b = mu_bias.  A plain layer is copied.  eps = 0 gives mu bit for bit (mu + 0 = mu).
 * tsm_noisy_grad replaces  autograd through the same lines.  One launch.  eff_slabs [n_split][P_eff] -> slabs [n_split][P],
 *   slab by slab:  d mu_W = dW;  d sigma_W = dW * (eps_q[o] * eps_p[i]);  d mu_bias = db;  d sigma_bias = db * eps_q[o]
 *   (training == 0: both sigma blocks +0.0);  the eps_p / eps_q slots +0.0;  a plain layer is copied.
 * tsm_dueling_combine replaces  `q - q.mean(dim=1, keepdim=True) + v` (common.py:360-364) on q [R][n_act][n_atoms],
 *   v [R][n_atoms]:  s = q[r][0][n] + q[r][1][n] + ... in action order, out[r][a][n] = (q[r][a][n] - s / n_act) + v[r][n].
 *   out is the raw [R][n_act * n_atoms] of tsm_distq_values / tsm_c51_head (bounds: tsm_distq_check).
 * tsm_dueling_combine_backward:  s = sum_a d[r][a][n] in action order;  d_q[r][a][n] = d[r][a][n] - s / n_act;  d_v[r][n] = s.
 * tsm_dueling_features replaces  the last activation of the dueling Net's trunk (`MLP(output_dim=0)` ends in its
 *   activation, a FlatMLP linearly): f = relu(z), n elements.
 * tsm_dueling_features_backward joins the two streams' input gradients (tsm_mlp_input_grad):
 *   d_z = z > 0 ? d_fq + d_fv : 0.
 * ------------------------------------------------------------------------------------------- */
#define TSM_NOISY_MAX_LAYERS 24
typedef struct tsm_noisy_layer {
    int64_t off, eff_off, slot_off;
    int32_t n_in, n_out, noisy, _pad;
} tsm_noisy_layer;
typedef struct tsm_noisy_net {
    int32_t n_layers, _pad;
    int64_t P, P_eff, n_slots;
    tsm_noisy_layer layer[TSM_NOISY_MAX_LAYERS];
} tsm_noisy_net;
int tsm_rainbow_check(const tsm_noisy_net *net);
int tsm_noisy_sample(const tsm_noisy_net *net, float *flat, uint64_t seed, uint64_t offset, const uint64_t *offset_dev,
                     void *stream);
int tsm_noisy_compose(const tsm_noisy_net *net, const float *flat, int training, float *eff, void *stream);
int tsm_noisy_grad(const tsm_noisy_net *net, const float *flat, const float *eff_slabs, int32_t n_split, int training,
                   float *slabs, void *stream);
int tsm_dueling_combine(const float *q, const float *v, int64_t R, int32_t n_act, int32_t n_atoms, float *out, void *stream);
int tsm_dueling_combine_backward(const float *d, int64_t R, int32_t n_act, int32_t n_atoms, float *d_q, float *d_v,
                                 void *stream);
int tsm_dueling_features(const float *z, int64_t n, float *f, void *stream);
int tsm_dueling_features_backward(const float *z, const float *d_fq, const float *d_fv, int64_t n, float *d_z, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Grouped ensemble MLP  (EnsembleLinear, tianshou/utils/net/common.py:522-554; csrc/ensemble.hip)
 * E networks of the shape `desc` as ONE launch per layer and role, the member a grid dimension; f32-input MFMA as
 * csrc/dense.hip.  params f32 [tsm_ens_mlp_param_count] in the reference's `parameters()` order, per layer
 * weight [E][dims[l]][dims[l + 1]] then bias_weights [E][1][dims[l + 1]] (a reference checkpoint is a set of views of it).
 * x f32 [B][dims[0]] is shared by all members; activation blocks are [E][B][dims[l]], layer after layer
 * (tsm_ens_mlp_act_elems floats); the output is the last block, [E][B][dims[L]].  No alignment is asked of any pointer or
 * width.  E in [1, TSM_ENS_MAX_MEMBERS] and desc as tsm_mlp_*: anything else is TSM_ERR_INVALID before any launch.
 * tsm_ens_mlp_backward: d_out [E][B][dims[L]]; d_acts: workspace of tsm_ens_mlp_act_elems floats (n_layers > 1);
 *   slabs [n_split][slab_stride] (slab_stride 0: the parameter count) receive the gradient in the parameter layout, every
 *   entry of every slab written: tsm_adam_step sums them.  E * n_split <= 65535 (one grid dimension).
 * tsm_ens_mlp_input_grad: the dgrad chain without weight gradients, ended by
 *   dx[b * ldx + j] = sum_e sum_o dZ0_e[b][o] W0_e[col0 + j][o], the members summed in the order e = 0 .. E - 1 inside one
 *   workgroup's k loop (one writer per element, no atomics).
 * Every sum has a fixed order: two runs give the same bits.
 * ------------------------------------------------------------------------------------------- */
#define TSM_ENS_MAX_MEMBERS 64
int64_t tsm_ens_mlp_param_count(const tsm_mlp_desc *desc, int32_t E);
int64_t tsm_ens_mlp_act_elems(const tsm_mlp_desc *desc, int32_t E, int64_t B);
int tsm_ens_mlp_forward(const tsm_mlp_desc *desc, int32_t E, const float *params, const float *x, int64_t B, float *acts,
                        void *stream);
int tsm_ens_mlp_backward(const tsm_mlp_desc *desc, int32_t E, const float *params, const float *x, int64_t B,
                         const float *acts, const float *d_out, float *d_acts, int32_t n_split, float *slabs,
                         int64_t slab_stride, void *stream);
int tsm_ens_mlp_input_grad(const tsm_mlp_desc *desc, int32_t E, const float *params, const float *x, int64_t B,
                           const float *acts, const float *d_out, float *d_acts, int32_t col0, int32_t n_col, float *dx,
                           int64_t ldx, void *stream);

/* ---------------------------------------------------------------------------------------------
 * REDQ  (tianshou/algorithm/modelfree/redq.py; csrc/redq.hip)
 * q f32 [E][B]: the ensemble critic's output.  One launch each, one thread per row walking the members in order, float64
 * arithmetic from the float32 inputs; the loss leaves as per-workgroup float64 pairs in tsm_qmix_mix_td's layout,
 * partial f64 [2 * ceil(B / TSM_REDQ_ROWS_PER_BLOCK)], for tsm_qmix_finalize(partial, n_blocks, E * B, ..).  No atomics.
 * tsm_redq_target replaces  _target_q_compute_value (redq.py:254-269) after the lagged ensemble's forward, and
 *           `_nstep_return`'s last line.  subset_mask: bit e set = member e is in the subset (at least one, none >= E);
 *   target_q = min (TSM_REDQ_MIN) or mean (TSM_REDQ_MEAN) over the subset - alpha logp_next (logp_next nullable: nothing);
 *   returns_out f32 [B] by tsm_dqn_td_head's rounding rule.
 * tsm_redq_critic_head replaces  redq.py:273-279 between the forward and optimizer.step.  td_e = q_e - returns;
 *   dq f32 [E][B] = 2 td_e weight / (E B) (weight [B] nullable: 1);  prio f32 [B] = mean_e td_e (signed);
 *   partial = {sum_e sum_b td_e^2 weight, 0}.
 * tsm_redq_mean_q: out f32 [B] = mean_e q[e][b]  (redq.py:287).
 * ------------------------------------------------------------------------------------------- */
#define TSM_REDQ_ROWS_PER_BLOCK 256
#define TSM_REDQ_MIN 0
#define TSM_REDQ_MEAN 1
int tsm_redq_target(const float *q_next, int32_t E, uint64_t subset_mask, int32_t mode, const float *logp_next,
                    const float *alpha_dev, const float *mc, const float *gpow, const uint8_t *vmask, int64_t B,
                    float *returns_out, void *stream);
int tsm_redq_critic_head(const float *q, int32_t E, const float *returns, const float *weight, int64_t B, float *dq,
                         float *prio, double *partial, void *stream);
int tsm_redq_mean_q(const float *q, int32_t E, int64_t B, float *out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * BDQN  (tianshou/algorithm/modelfree/bdqn.py, BranchingNet in tianshou/utils/net/common.py:557-678; csrc/bdqn.hip)
 * K branches of A actions each.  adv f32 [K][B][A]: the grouped ensemble's output block (tsm_ens_mlp_forward with E = K);
 * v f32 [B]; q f32 [B][K][A]: the reference's logits; act i32 [B][K].  K in [1, TSM_ENS_MAX_MEMBERS], A in [1, 64] (DQN's
 * bound), B as tsm_dqn_td_head: anything else, or a null pointer where none is allowed, is TSM_ERR_INVALID naming the limit
 * before any launch (tsm_bdqn_check: the two bounds alone).  Float64 arithmetic from the float32 inputs, every sum in a fixed
 * order, no atomics: two runs give the same bits.
 * tsm_bdqn_combine replaces  BranchingNet.forward after its MLPs (common.py:669-677):
 *   q[b][k][a] = v[b] + (adv[k][b][a] - mean_a' adv[k][b][a']), the mean summed a' = 0 .. A - 1.
 * tsm_bdqn_head replaces  _target_q after its forwards (bdqn.py:155-171), _compute_return (:173-195) and _update_with_batch
 *           between `self.policy(batch).logits` and `optim.step` (:211-221), in one launch.
 *   q_next_target nullable: the online values are the target values.  a*_k = the first maximum of q_next_online[b][k][:]
 *   (is_double) or of the target values;  tq_b = mean_k target[b][k][a*_k], k in order;
 *   returns[b] = rew[b] + gamma tq_b (1 - end[b]), rounded to f32 once (tsm_dqn_td_head's rule; end u8: terminated or
 *   truncated or the sub-buffer's newest row);  td_bk = returns[b] - q[b][k][act[b][k]];
 *   loss = mean_b(w_b mean_k td_bk^2) (weight [B] nullable: 1);  prio f32 [B] = sum_k td_bk (signed);
 *   g_bk = -2 w_b td_bk / (K B);  d_adv f32 [K][B][A] = g_bk ((a == act[b][k]) - 1 / A);  d_v f32 [B] = sum_k g_bk: the
 *   combine's backward is folded in, d_adv feeds tsm_ens_mlp_backward / _input_grad, d_v the value stream.
 *   partial f64 [2 * ceil(B / TSM_BDQN_ROWS_PER_BLOCK)] = {sum_b w_b mean_k td^2, sum_b mean_k q[b][k][act]} per workgroup in
 *   tsm_qmix_mix_td's layout, for tsm_qmix_finalize(partial, n_blocks, B, ..).
 *   An act entry outside [0, A) reads nothing, as in tsm_dqn_td_head: its td is NaN (loss and prio[b] are poisoned), its
 *   d_adv row and its share of d_v are 0.
 * tsm_bdqn_egreedy replaces  BDQNPolicy.forward's argmax (:76) and add_exploration_noise (:80-103).  q [R][K][A] ->
 *   act_out i32 [R][K].  One coin per row: row r draws at Philox counter offset + *offset_dev + r; random where
 *   u01(word 0 of sub 0) < *eps_dev in float32, then branch k takes (word k % 4 of sub 1 + k / 4) * A >> 32; else every branch
 *   takes its first maximum.  No word is shared between rows, branches or the coin.  (`rand_act += batch.obs.mask` is not
 *   reproduced: the Python policy refuses masked observations.)
 * ------------------------------------------------------------------------------------------- */
#define TSM_BDQN_ROWS_PER_BLOCK 16
int tsm_bdqn_check(int32_t K, int32_t A);
int tsm_bdqn_combine(const float *adv, const float *v, int64_t B, int32_t K, int32_t A, float *q, void *stream);
int tsm_bdqn_head(const float *q, const float *q_next_online, const float *q_next_target, const int32_t *act,
                  const float *rew, const uint8_t *end, const float *weight, int64_t B, int32_t K, int32_t A, double gamma,
                  int is_double, float *returns_out, float *prio, float *d_adv, float *d_v, double *partial, void *stream);
int tsm_bdqn_egreedy(const float *q, int64_t R, int32_t K, int32_t A, const float *eps_dev, uint64_t seed, uint64_t offset,
                     const uint64_t *offset_dev, int32_t *act_out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * ICM  (tianshou/algorithm/modelbased/icm.py, IntrinsicCuriosityModule in tianshou/utils/net/discrete.py:378-429;
 * csrc/icm.hip)
 * Three MLPs (csrc/dense.hip) around one row-wise head.  The feature net runs ONCE over 2R interleaved rows, obs of row r at
 * 2r and obs_next at 2r + 1: phi f32 [2R][feature_dim], so phi1[r] = phi[2r], phi2[r] = phi[2r + 1], and phi viewed as
 * [R][2 feature_dim] is [phi1 | phi2], the inverse model's input, without a copy.  act i64 [R].  feature_dim in [1, 512], n_act
 * in [1, 64] as for tsm_dqn_check, R (2 feature_dim + n_act) below 2^31: anything else, or a null pointer where none is
 * allowed, is TSM_ERR_INVALID naming the limit before any launch.  Float64 arithmetic from the float32 inputs, rounded once
 * where a value leaves; a row sum is every lane's columns l, l + 64, .. in index order, then the xor butterfly; no atomics:
 * two runs give the same bits (the rule of the tsm_dsac_* heads).
 * tsm_icm_check: the two bounds alone.  Needs no device.
 * tsm_icm_rows replaces  torch.cat([phi1, F.one_hot(act, num_classes=action_dim)], dim=1) (discrete.py:424-426).  One launch.
 *   out: x_fwd f32 [R][feature_dim + n_act] = [phi[2r] | one_hot(act[r])], the forward model's input.  An action outside
 *   [0, n_act) gives an all-zero one-hot (the reference's F.one_hot raises).
 * tsm_icm_head replaces  `0.5 * F.mse_loss(phi2_hat, phi2, reduction="none").sum(1)` (discrete.py:427), `batch.rew +=
 *           mse_loss * reward_scale` (icm.py:83) and the loss of _icm_update with its backward down to the three networks'
 *           outputs (icm.py:95-101).  One launch, one wave per row.
 *   phi2_hat f32 [R][feature_dim]: the forward model on x_fwd; phi2: row r at phi2 + r * phi2_row_stride (phi + feature_dim
 *   with stride 2 feature_dim); act_hat f32 [R][n_act]: the inverse model on phi as [R][2 feature_dim].
 *   rew_io f32 (nullable: no store), ids i64 [R] (nullable): row r's reward lives at rew_io[ids ? ids[r] : r]; the ids are the
 *   caller's to keep inside rew_io and distinct (one writer per element).
 *   With d = phi2_hat - phi2, w = forward_loss_weight, s = lr_scale:
 *   out: mse f32 [R] = 0.5 sum_k d[k]^2;  rew_io[..] += (float)mse * (float)reward_scale, a float32 product and a float32 add;
 *        d_phi2_hat f32 [R][feature_dim] = s w d / R;  d_phi2_fwd f32 [R][feature_dim] = its negative (nothing is detached:
 *        the forward loss reaches phi2 too);
 *        d_act_hat f32 [R][n_act] = s (1 - w) (softmax(act_hat) - one_hot(act)) / R;
 *        partial f64 [2 * ceil(R / TSM_ICM_ROWS_PER_BLOCK)] = per workgroup {sum mse, sum ce}, ce = logsumexp(act_hat) -
 *        act_hat[act], both before their rounding to float32, in the layout of tsm_qmix_mix_td's partials:
 *        tsm_qmix_finalize(partial, n_blocks, R, out) gives out[2] = {icm_forward_loss, icm_inverse_loss};
 *        icm_loss = ((1 - w) icm_inverse_loss + w icm_forward_loss) s follows from the two in float64 on the host.
 *   An action outside [0, n_act) reads nothing, as in tsm_dsac_critic_head: the row's mse and ce (and what its reward takes) are
 *   NaN, its three gradient rows zero.  s = 0 gives exact zeros in all three gradients, w = 0 in the two forward ones, w = 1 in
 *   d_act_hat.
 * tsm_icm_join_grad: the feature net's d_out f32 [2R][feature_dim] in one launch.
 *   g_fwd f32 [R][feature_dim]: the forward model's input gradient, columns [0, feature_dim) (tsm_mlp_input_grad);
 *   g_inv f32 [R][2 feature_dim]: the inverse model's input gradient; d_phi2_fwd from tsm_icm_head.
 *   d_out[2r] = g_fwd[r] + g_inv[r][0 .. feature_dim);  d_out[2r + 1] = g_inv[r][feature_dim ..) + d_phi2_fwd[r]: float32 sums
 *   in that written order.  d_out may be g_inv itself (the two share their layout; every element has one reader and writer).
 * ------------------------------------------------------------------------------------------- */
#define TSM_ICM_ROWS_PER_BLOCK 16
int tsm_icm_check(int32_t feature_dim, int32_t n_act);
int tsm_icm_rows(const float *phi, const int64_t *act, int64_t R, int32_t feature_dim, int32_t n_act, float *x_fwd,
                 void *stream);
int tsm_icm_head(const float *phi2_hat, const float *phi2, int64_t phi2_row_stride, const float *act_hat, const int64_t *act,
                 float *rew_io, const int64_t *ids, int64_t R, int32_t feature_dim, int32_t n_act, double reward_scale,
                 double forward_loss_weight, double lr_scale, float *mse, float *d_phi2_hat, float *d_phi2_fwd,
                 float *d_act_hat, double *partial, void *stream);
int tsm_icm_join_grad(const float *g_fwd, const float *g_inv, const float *d_phi2_fwd, int64_t R, int32_t feature_dim,
                      float *d_out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * GAIL  (tianshou/algorithm/imitation/gail.py; csrc/gail.hip)
 * PPO whose reward is -logsigmoid(-D([obs | act])) of a discriminator D (an MLP of csrc/dense.hip ending in one logit), trained
 * by a few steps per update against an expert buffer.  A "pair" is one (buffer row, agent) sample; its id p is the flat index
 * into obs_store viewed as [S B N][obs_dim], act_store viewed as i32 [S B N] and rew_store viewed as [S B N]: the kernels read
 * the stores in place.  The action enters one-hot (the reference concatenates batch.act as it is, which serves Box actions
 * only).  n_act in [1, 64] as for tsm_dqn_check, obs_dim >= 1, R (obs_dim + n_act) below 2^31 (R >= 1): anything else, or a null
 * pointer where none is allowed, is TSM_ERR_INVALID naming the limit before any launch.  Float64 arithmetic from the float32
 * inputs, rounded once where a value leaves; a workgroup's sum is every wave's xor butterfly over its 64 rows, then the waves
 * in order (tsm_icm_head's rule); no atomics: two runs give the same bits.
 * softplus(x) = max(x, 0) + log1p(exp(-|x|));  sigmoid(x) = 1 / (1 + exp(-x)) for x >= 0, exp(x) / (1 + exp(x)) below.
 * tsm_gail_check: the bounds alone.  Needs no device.
 * tsm_gail_draw replaces  expert_buffer.sample(bsz) (gail.py:227; uniform with replacement).  Element i takes Philox word 0 at
 *   counter `counter + *counter_dev + i` (counter_dev nullable: 0) under the key seed ^ kGailKey (0x4741494C45585054, which no
 *   other site uses); j = (w0 * (n_valid n_agent)) >> 32, the tsm_qmix_egreedy integer rule;
 *   ids_out i64 [R]: [i] = (valid ? valid[j / n_agent] : j / n_agent) * n_agent + j % n_agent.  valid i64 [n_valid] (nullable: the
 *   rows 0 .. n_valid - 1): the expert buffer's store rows that hold data.  n_valid n_agent in [1, 2^32).
 * tsm_gail_rows replaces  torch.cat([obs, act], dim=1) (gail.py:208-212) on one-hot actions.  One launch.
 *   out: x_out f32 [R][obs_dim + n_act] = [obs[p] | one_hot(act[p])], p = ids ? ids[r] : r (ids i64 [R] nullable).  An action
 *   outside [0, n_act) gives an all-zero one-hot, as in tsm_icm_rows.  The learner calls it for the policy rows and for the
 *   expert rows, each call writing its half of ONE matrix, so the discriminator runs once per step.
 * tsm_gail_reward replaces  batch.rew = -F.logsigmoid(-disc(batch)) (gail.py:204-205).
 *   rew_io[ids ? ids[r] : r] = (float)softplus(logits[r]): an overwrite.  The ids are the caller's to keep inside rew_io and
 *   distinct.
 * tsm_gail_head replaces  gail.py:226-235 and the backward of loss_disc down to the logits.  One launch.
 *   logits f32 [Rp + Re]: the policy rows, then the expert rows; Rp, Re >= 1 may differ (merge_last makes the last policy chunk
 *   longer).  d_logits f32 [Rp + Re] = sigmoid(l) / Rp for a policy row, (sigmoid(l) - 1) / Re for an expert row, formed as
 *   -sigmoid(-l) / Re: no cancellation at large l.
 *   partial f64 [4 * ceil((Rp + Re) / TSM_GAIL_ROWS_PER_BLOCK)] = per workgroup {sum softplus(l_pi), sum softplus(-l_exp),
 *   count(l_pi < 0), count(l_exp > 0)}.
 * tsm_gail_finalize: out f32 [3] (device or mapped host memory) = {loss_pi / Rp + loss_exp / Re, acc_pi, acc_exp} of one step,
 *   the block sums added in index order.
 * ------------------------------------------------------------------------------------------- */
#define TSM_GAIL_ROWS_PER_BLOCK 256
int tsm_gail_check(int32_t obs_dim, int32_t n_act);
int tsm_gail_draw(const int64_t *valid, int64_t n_valid, int32_t n_agent, int64_t R, uint64_t seed, uint64_t counter,
                  const uint64_t *counter_dev, int64_t *ids_out, void *stream);
int tsm_gail_rows(const float *obs, const int32_t *act, const int64_t *ids, int64_t R, int32_t obs_dim, int32_t n_act,
                  float *x_out, void *stream);
int tsm_gail_reward(const float *logits, const int64_t *ids, int64_t R, float *rew_io, void *stream);
int tsm_gail_head(const float *logits, int64_t Rp, int64_t Re, float *d_logits, double *partial, void *stream);
int tsm_gail_finalize(const double *partial, int64_t n_blocks, int64_t Rp, int64_t Re, float *out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Learned global states  (tianshou/algorithm/multiagent/ctde.py:230-343, GlobalStateConstructor modes "attention" and
 * "graph"; csrc/gstate.hip)
 * What lies between the modes' matrix products with weights, which stay on csrc/dense.hip.  A row is one joint step, its N
 * agents in env.agents order.  1 <= N <= TSM_GSTATE_MAX_AGENTS; D % TSM_GSTATE_HEADS == 0 and TSM_GSTATE_HEADS <= D <=
 * TSM_GSTATE_MAX_DIM (a head is dh = D / 4 <= 64 wide); H >= 1; B >= 1: anything else, or a null pointer where none is allowed,
 * is TSM_ERR_INVALID naming the limit before any launch.  Float32 arithmetic; every sum is taken by one lane in index order, no
 * atomics: two runs give the same bits.
 * tsm_gstate_check: the bounds on (N, D) alone.  Needs no device.
 * tsm_attn_pool_forward replaces  the core of nn.MultiheadAttention(embed_dim = D, num_heads = 4, batch_first = True) between
 *   its in- and out-projection, and the mean over agents behind it (ctde.py:270-274, 308-311), without mask or dropout.
 *   qkv f32 [B][N][3 D], 16-byte aligned (it is staged with 16-B loads; rows are multiples of 16 B as D % 4 == 0): the
 *   in-projection of agent n's observation, [Q | K | V].  Per row and head h (columns h dh .. h dh + dh
 *   of each part):  S = (Q_h / sqrt(dh)) K_h^T  [N][N];  P = softmax over the keys, the row maximum subtracted;  O = P V_h.
 *   out: ctx f32 [B][D] = (1 / N) sum_n concat_h(O)[n] (the mean is taken BEFORE the out-projection, which is linear:
 *   mean_n(W O_n + b) = W mean_n O_n + b), formed as sum_j ((sum_i P[h][i][j]) V[j][d]) / N;  P f32 [B][4][N][N] for the backward.
 *   TSM_GSTATE_ROWS_PER_BLOCK rows per workgroup, one wave each.
 * tsm_attn_pool_backward: d_ctx f32 [B][D], qkv and P as above -> d_qkv f32 [B][N][3 D], every element written:
 *   d P[h][i][j] = (1 / N) sum_t d_ctx[h dh + t] V[j][h dh + t] (the same for every query i);  d S = P (d P - sum_j P d P);
 *   d Q[i] = sum_j d S[i][j] K[j] / sqrt(dh);  d K[j] = sum_i d S[i][j] Q[i] / sqrt(dh);  d V[j][d] = (d_ctx[d] / N) sum_i P[h][i][j].
 * tsm_agent_pool_forward replaces  the neighbour aggregation and the mean over agents of mode "graph" (ctde.py:320-335) around
 *   gnn_layer2, which is linear:  mean_n(W2 (A^ x)_n + b2) = W2 (sum_m c_m x_m) + b2,  c_m = (1 / N) sum_n A^[n][m], A^ the
 *   row-normalised adjacency (no adjacency: c_m = 1 / N).  h f32 [B][N][H], c f32 [N] (device) ->
 *   out f32 [B][H] = sum_n c[n] f(h[b][n][:]), n in order;  relu != 0: f = max(., 0), the F.relu of ctde.py:320 behind
 *   gnn_layer1, whose dense.hip net ends linear;  relu == 0: f the identity.
 * tsm_agent_pool_backward: d f32 [B][H] -> d_h f32 [B][N][H] = c[n] d[b][:], times 1[h_relu[b][n][:] > 0] where h_relu (the
 *   forward's h, nullable) is given.
 * ------------------------------------------------------------------------------------------- */
#define TSM_GSTATE_MAX_AGENTS 8
#define TSM_GSTATE_HEADS 4
#define TSM_GSTATE_MAX_DIM 256
#define TSM_GSTATE_ROWS_PER_BLOCK 4
int tsm_gstate_check(int32_t n_agents, int32_t obs_dim);
int tsm_attn_pool_forward(const float *qkv, int64_t B, int32_t n_agents, int32_t D, float *ctx, float *P, void *stream);
int tsm_attn_pool_backward(const float *d_ctx, const float *qkv, const float *P, int64_t B, int32_t n_agents, int32_t D,
                           float *d_qkv, void *stream);
int tsm_agent_pool_forward(const float *h, const float *c, int64_t B, int32_t n_agents, int32_t H, int32_t relu, float *out,
                           void *stream);
int tsm_agent_pool_backward(const float *d, const float *c, const float *h_relu, int64_t B, int32_t n_agents, int32_t H,
                            float *d_h, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Recurrent Q-learning  (tianshou/utils/net/common.py:372-458 `Recurrent`; data/buffer/buffer_base.py:495-590 frame stacking;
 * csrc/lstm.hip, csrc/dense.hip, csrc/vrb.hip)
 * tsm_dense_linear / _dgrad / _wgrad: the three row GEMMs of ONE linear layer with its operands given apart (the engine of
 *   tsm_mlp_*, f32 MFMA), for parameters that do not lie as W | b pairs and for strided rows:
 *     linear  out[M][O] = x[M][K (row pitch ldx)] W[O][K]^T + bias[O]
 *     dgrad   dx[M][K (row pitch ld_dx)] = dz[M][O] W[O][K]
 *     wgrad   slab z of n_split, at slabs + z * slab_stride: [w_off + o * K + k] = sum over the slab's rows of dz[m][o] x[m][k],
 *             [b_off + o] = sum of dz[m][o]; the rows are dealt to the slabs as by tsm_mlp_backward, the slabs sum to the gradient.
 * The LSTM layer: torch's layout, gate order i, f, g, o; weight_hh [4H][H].  H a multiple of 16 in [16, TSM_LSTM_MAX_HIDDEN],
 *   layer_num >= 1, L >= 1, B >= 1: anything else is TSM_ERR_INVALID from tsm_lstm_check (needs no device) before any launch.
 *   A workgroup carries TSM_LSTM_ROWS_PER_BLOCK batch rows through all L steps: one launch per layer and direction.
 * tsm_lstm_forward: proj f32 [B][L][4H] = X W_ih^T + b_ih (tsm_dense_linear); bias (nullable) [4H] is added to it (b_hh);
 *   h0, c0 (nullable: zeros) and h_n, c_n (nullable) are [B] rows of H floats at row pitch ld_state (a layer's slice of a
 *   [B][layers][H] state); h_n / c_n may be h0 / c0 themselves (the acting step, L = 1, advances the state in place).
 *   Per step: gates = proj_t + bias + h_{t-1} W_hh^T;  i, f, o = sigmoid, g = tanh;  c_t = f c_{t-1} + i g;  h_t = o tanh(c_t).
 *   out: h [B][L][H]; for the backward (each nullable) h_prev [B][L][H] = h_{t-1}, gates [B][L][4H] activated, c [B][L][H].
 *   sigmoid and tanh are finite for every finite input.
 * tsm_lstm_backward: d_h [B][L][H] = the gradient arriving at every h_t from above; d_hn, d_cn (nullable) at h_L, c_L;
 *   gates, c as saved; c0 as given to the forward -> d_gates [B][L][4H] w.r.t. the pre-activations, every element written,
 *   and (nullable) d_h0, d_c0.  d_h_{t-1} += d_gates_t W_hh on f32 MFMA.  The weight gradients are then
 *   tsm_dense_wgrad(d_gates, X) -> weight_ih, bias_ih and tsm_dense_wgrad(d_gates, h_prev) -> weight_hh, bias_hh, and the
 *   gradient for the layer below tsm_dense_dgrad(d_gates, W_ih).
 * tsm_lstm_state_reset: h, c f32 [n_env * rows_per_env][row_elems]; the rows of env e are zeroed where done[e] != 0
 *   (collector.py:977-979).  One launch, no host read: safe inside a captured graph.
 * tsm_vrb_gather_stacked replaces  ReplayBuffer.get(index, key, stack_num) (buffer_base.py:533-590): stack_num - 1 rounds of
 *   tsm_vrb_prev's rule from index[i], then out[i][l] = bytes [lane_off, lane_off + lane_bytes) of the store row of the
 *   (stack_num - 1 - l)-th predecessor: oldest first, a frame repeating where the walk stops at an episode start or the oldest
 *   row.  out [n][stack_num][lane_bytes].  Bit-identical to stack_num rounds of tsm_vrb_prev + tsm_vrb_gather.  One launch.
 * ------------------------------------------------------------------------------------------- */
#define TSM_LSTM_MAX_HIDDEN 128
#define TSM_LSTM_ROWS_PER_BLOCK 16
int tsm_dense_linear(const float *x, int64_t ldx, const float *W, const float *bias, int64_t M, int32_t K, int32_t O, float *out,
                     void *stream);
int tsm_dense_dgrad(const float *dz, const float *W, int64_t M, int32_t O, int32_t K, float *dx, int64_t ld_dx, void *stream);
int tsm_dense_wgrad(const float *dz, const float *x, int64_t ldx, int64_t M, int32_t O, int32_t K, int32_t n_split, float *slabs,
                    int64_t slab_stride, int64_t w_off, int64_t b_off, void *stream);
int tsm_lstm_check(int32_t hidden, int32_t layer_num, int32_t seq_len);
int tsm_lstm_forward(const float *proj, const float *w_hh, const float *bias, const float *h0, const float *c0, int64_t ld_state,
                     int64_t B, int32_t L, int32_t H, float *h, float *h_prev, float *gates, float *c, float *h_n, float *c_n,
                     void *stream);
int tsm_lstm_backward(const float *d_h, const float *d_hn, const float *d_cn, const float *w_hh, const float *gates,
                      const float *c, const float *c0, int64_t ld_state, int64_t B, int32_t L, int32_t H, float *d_gates,
                      float *d_h0, float *d_c0, void *stream);
int tsm_lstm_state_reset(float *h, float *c, const uint8_t *done, int64_t n_env, int64_t rows_per_env, int64_t row_elems,
                         void *stream);
int tsm_vrb_gather_stacked(const void *state, int64_t buffer_num, int64_t sub_size, const uint8_t *done_store, const void *store,
                           int64_t row_bytes, int64_t lane_off, int64_t lane_bytes, const int64_t *index, int64_t n,
                           int32_t stack_num, void *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TSMARL_H */
