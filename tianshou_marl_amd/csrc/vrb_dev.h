// vrb_dev.h -- device-side VectorReplayBuffer index algebra shared by vrb.hip and the persistent rollout
// kernel.  Restates ReplayBuffer._update_state_pre_add + ReplayBufferManager.add
// (/root/reference/tianshou/data/buffer/buffer_base.py:355-410, manager.py:159-177); bit-exact with the
// reference (tests/test_gpu_kernels.py::test_vrb_trace_bit_exact).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct VrbState {
    int64_t *ins, *size, *ep_len, *ep_start, *last_index, *lengths;
    double *ep_return;
    int64_t *error_flag;
};

// state = i64 insertion_idx[B] size[B] ep_len[B] ep_start_idx[B] last_index[B] lengths[B] | f64 ep_return[B][D] | i64 flag
__host__ __device__ inline VrbState vrb_view(void *state, int64_t B, int64_t D) {
    VrbState s;
    int64_t *p = reinterpret_cast<int64_t *>(state);
    s.ins = p;
    s.size = p + B;
    s.ep_len = p + 2 * B;
    s.ep_start = p + 3 * B;
    s.last_index = p + 4 * B;
    s.lengths = p + 5 * B;
    s.ep_return = reinterpret_cast<double *>(p + 6 * B);
    s.error_flag = p + 6 * B + B * D;
    return s;
}

// Index bookkeeping for ONE row added to sub-buffer `e`.  Returns the slot the payload goes to.
// Outputs: *ptr_out (flat reference index), ep_rew_out[D], *ep_len_out, *ep_idx_out  (manager.py:193).
__device__ inline int64_t vrb_add_row(const VrbState &s, int64_t B, int64_t S, int64_t D, int64_t e,
                                      const float *rew_row, bool d, uint8_t *done_store, int64_t *ptr_out,
                                      double *ep_rew_out, int64_t *ep_len_out, int64_t *ep_idx_out) {
    const int64_t cur = s.ins[e];                        // buffer_base.py:373
    int64_t sz = s.size[e] + 1; if (sz > S) sz = S;       // :374
    int64_t nxt = cur + 1; if (nxt >= S) nxt -= S;        // :375
    const int64_t elen = s.ep_len[e] + 1;                 // :378
    const int64_t estart = s.ep_start[e];
    if (estart > sz) atomicExch((unsigned long long *)s.error_flag, 1ull);  // :380-386
    for (int64_t k = 0; k < D; ++k) {
        const double acc = s.ep_return[e * D + k] + (double)rew_row[k];      // :377
        ep_rew_out[k] = d ? acc : 0.0;                    // :389-402
        s.ep_return[e * D + k] = d ? 0.0 : acc;           // :409
    }
    *ep_len_out = d ? elen : 0;
    const int64_t off = e * S;
    *ptr_out = cur + off;                                 // manager.py:170
    *ep_idx_out = estart + off;                           // manager.py:171
    s.ins[e] = nxt;
    s.size[e] = sz;
    s.ep_len[e] = d ? 0 : elen;
    s.ep_start[e] = d ? nxt : estart;                     // :409
    s.last_index[e] = cur + off;                          // manager.py:176
    s.lengths[e] = sz;                                    // manager.py:177
    done_store[cur * B + e] = d ? 1 : 0;
    return cur;
}

// The same bookkeeping for the persistent rollout kernels: the sub-buffer state of "my" env lives in the registers of one lane
// (the env lane) for the whole rollout, so a step's index algebra has no dependent global loads, only fire-and-forget stores.
// (vrb_add_row above stays the unfused path these kernels are tested against: it does not go through this type.)
struct VrbStep {
    int64_t row;  // slot * B + env: where the step's payload rows go
    int64_t o;    // t * B + env: the step's place in the per-step outputs
    bool rec;     // the episode that ends here gets an ep_rec entry (index n_fin)
};

struct VrbLane {
    int64_t ins = 0, size = 0, ep_len = 0, ep_start = 0, last = 0;   // zero: a lane that owns no env
    int n_fin = 0;   // episodes this env finished during the rollout; counted by the caller (a kernel may keep a second count on
                     // the lanes that fold the episode returns)

    __device__ __forceinline__ void load(const VrbState &vs, int be) {
        ins = vs.ins[be]; size = vs.size[be]; ep_len = vs.ep_len[be]; ep_start = vs.ep_start[be];
        last = vs.last_index[be];
    }

    // Row t of env `be` (tr: its episode ends here): buffer_base.py:373-410 + manager.py:170-177, same arithmetic as vrb_add_row.
    // The outputs are [n_steps][B] arrays; ep_rec (nullable, max_ep entries per env) is the rollout's compact episode record.
    // (Pointers and sizes come by value: handing the kernel's argument struct over by reference made every field of it a load
    //  the compiler may hoist to the kernel's entry -- rollout_tag_kernel 184 -> 199 VGPRs, 234 -> 288 spilled scalar registers.)
    __device__ __forceinline__ VrbStep add(const VrbState &vs, int64_t S, int t, int be, int64_t B, bool tr, uint8_t *done_store,
                                           int64_t *ptr_out, int64_t *ep_len_out, int64_t *ep_idx_out, int64_t *ep_rec, int max_ep) {
        VrbStep s;
        s.o = (int64_t)t * B + be;
        const int64_t cur = ins;
        int64_t sz = size + 1; if (sz > S) sz = S;
        int64_t nxt = cur + 1; if (nxt >= S) nxt -= S;
        const int64_t elen = ep_len + 1;
        if (ep_start > sz) atomicExch((unsigned long long *)vs.error_flag, 1ull);
        s.rec = tr && ep_rec && n_fin < max_ep;
        // (the record carries CollectStats.lens = len(episode_batch): the episode's rows IN THE BUFFER, collector.py:203,990-993 --
        //  after a reset_buffer(keep_statistics=True) an episode counts its rows since the reset; ep_len_out stays add()'s ep_len)
        if (s.rec) ep_rec[B + (int64_t)be * max_ep + n_fin] = ((int64_t)t << 32) | ((cur >= ep_start ? cur - ep_start : cur - ep_start + S) + 1);
        ep_len_out[s.o] = tr ? elen : 0;
        ptr_out[s.o] = cur + (int64_t)be * S;
        ep_idx_out[s.o] = ep_start + (int64_t)be * S;
        ins = nxt; size = sz; ep_len = tr ? 0 : elen; ep_start = tr ? nxt : ep_start;
        last = cur + (int64_t)be * S;
        done_store[cur * B + be] = tr ? 1 : 0;
        s.row = cur * B + be;
        return s;
    }

    __device__ __forceinline__ void store(const VrbState &vs, int64_t *ep_rec, int be) const {
        vs.ins[be] = ins; vs.size[be] = size; vs.ep_len[be] = ep_len; vs.ep_start[be] = ep_start;
        vs.last_index[be] = last; vs.lengths[be] = size;
        if (ep_rec) ep_rec[be] = n_fin;  // may exceed max_ep: the host treats that as an overflow
    }
};
