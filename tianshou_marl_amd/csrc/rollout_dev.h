// rollout_dev.h -- what the persistent rollout kernels (rollout.hip, rollout_rows.hip, rollout_tag.hip) share and that has nothing
// to do with how a kernel maps a step onto its waves: the buffer / output / counter arguments and their checks, the episode-return
// fold on the lanes that own an env, the advance of the sampling counter.  The env lane's sub-buffer state is VrbLane (vrb_dev.h).
// Everything a kernel calls is __forceinline__, takes its own state by reference and the kernel's arguments by value (see
// VrbLane::add): several of these kernels sit at the register limit.
#pragma once
#include "common.h"
#include "vrb_dev.h"

struct RolloutBufArgs {
    // buffer
    void *vrb_state;
    int64_t S;
    uint8_t *done_store;
    float *obs_store, *obs_next_store, *rew_store, *logp_store, *vs_store, *vnext_store;
    int32_t *act_store;
    uint8_t *term_store, *trunc_store;
    // per-step outputs [n_steps][n_env]...
    int64_t *ptr_out, *ep_len_out, *ep_idx_out;
    double *ep_rew_out;
    int n_steps;
    // compact record of the episodes finished during this rollout (nullable): i64 words
    //   [n_env] count | [n_env][max_ep] (step << 32 | length) | [n_env][max_ep][N] f64 return
    int64_t *ep_rec;
    int max_ep;
    uint64_t offset_inc;
    uint64_t *offset_dev_rw;
    uint32_t *done_ctr;
};

// tsm_rollout_desc / tsm_rollout_tag_desc -> the kernels' buffer arguments; `entry` names the caller in the messages
template <class Desc>
int rollout_buf_args(const Desc &h, const char *entry, RolloutBufArgs *b) {
    TSM_REQUIRE(h.vrb_state && h.done_store && h.obs_store && h.act_store && h.rew_store && h.term_store && h.trunc_store &&
                    h.ptr_out && h.ep_rew_out && h.ep_len_out && h.ep_idx_out,
                "%s: null pointer", entry);
    b->vrb_state = h.vrb_state; b->S = h.sub_size; b->done_store = h.done_store;
    b->obs_store = h.obs_store; b->obs_next_store = h.obs_next_store; b->rew_store = h.rew_store;
    b->logp_store = h.logp_store; b->vs_store = h.vs_store; b->vnext_store = h.vnext_store;
    b->act_store = h.act_store; b->term_store = h.term_store; b->trunc_store = h.trunc_store;
    b->ptr_out = h.ptr_out; b->ep_len_out = h.ep_len_out; b->ep_idx_out = h.ep_idx_out; b->ep_rew_out = h.ep_rew_out;
    b->n_steps = h.n_steps;
    TSM_REQUIRE(!h.ep_rec || h.max_ep >= 1, "%s: ep_rec needs max_ep >= 1", entry);
    b->ep_rec = h.ep_rec; b->max_ep = h.max_ep;
    TSM_REQUIRE(!h.done_ctr || h.offset_dev, "%s: done_ctr needs offset_dev", entry);
    b->offset_inc = h.offset_inc; b->done_ctr = h.done_ctr;
    b->offset_dev_rw = const_cast<uint64_t *>(reinterpret_cast<const uint64_t *>(h.offset_dev));
    return TSM_OK;
}

// The running episode returns of one env (f64, one per agent; MAXN: kMpeMaxN / kTagMaxAgents) on the lane that folds them.
template <int MAXN>
struct EpReturns {
    double acc[MAXN];

    __device__ __forceinline__ EpReturns() {   // zero: a lane that owns no env
#pragma unroll
        for (int k = 0; k < MAXN; ++k) acc[k] = 0.0;
    }
    __device__ __forceinline__ void load(const VrbState &vs, int N, int64_t be) {
#pragma unroll
        for (int k = 0; k < MAXN; ++k) if (k < N) acc[k] = vs.ep_return[be * N + k];
    }
    // Step `o` (= t * B + be, VrbStep::o) of env be from its agents' rewards `rew` (buffer_base.py:377,389-409): tr = the episode
    // ends here, rec = it gets the ep_rec entry n_fin (VrbStep::rec); counts the episode in n_fin.
    __device__ __forceinline__ void fold(double *ep_rew_out, int64_t *ep_rec, int max_ep, int N, int64_t B, int64_t be, int64_t o, bool tr,
                                         bool rec, int &n_fin, const float *rew) {
        double *rec_rew = rec ? reinterpret_cast<double *>(ep_rec + B + (int64_t)B * max_ep) +
                                    ((int64_t)be * max_ep + n_fin) * N : nullptr;
#pragma unroll
        for (int k = 0; k < MAXN; ++k) {
            if (k < N) {
                const double ac = acc[k] + (double)rew[k];
                ep_rew_out[o * N + k] = tr ? ac : 0.0;
                if (rec) rec_rew[k] = ac;
                acc[k] = tr ? 0.0 : ac;
            }
        }
        n_fin += tr ? 1 : 0;
    }
    __device__ __forceinline__ void store(const VrbState &vs, int N, int64_t be) const {
#pragma unroll
        for (int k = 0; k < MAXN; ++k) if (k < N) vs.ep_return[be * N + k] = acc[k];
    }
};

// The last workgroup to get here advances the sampling counter: every workgroup has read it before finishing.  Called at the very
// end of the kernel; `first` = this is the workgroup's thread 0.
// n_wg: the workgroups that arrive here (a launch may carry others that never read the counter).
__device__ __forceinline__ void rollout_advance_counter(uint32_t *done_ctr, uint64_t *offset_dev_rw, uint64_t offset_inc, bool first,
                                                        unsigned n_wg) {
    if (done_ctr && first) {
        if (atomicAdd(done_ctr, 1u) == n_wg - 1) {
            *offset_dev_rw += offset_inc;
            *done_ctr = 0u;
        }
    }
}
__device__ __forceinline__ void rollout_advance_counter(uint32_t *done_ctr, uint64_t *offset_dev_rw, uint64_t offset_inc, bool first) {
    rollout_advance_counter(done_ctr, offset_dev_rw, offset_inc, first, gridDim.x);
}
