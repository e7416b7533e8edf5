// rainbow.hip -- Rainbow's network side: NoisyLinear layers (the noise draw, the effective weights, the gradient map back) and
// the dueling Q / V streams (the trunk's last activation, the combine, both backward).
//
// Replaces NoisyLinear.sample / .f / the weight lines of .forward (tianshou/utils/net/discrete.py:358-373) with
// autograd through them, and `q - q.mean(dim=1, keepdim=True) + v` of Net.forward (utils/net/common.py:360-364) with the last
// activation of the dueling Net's trunk (`MLP(output_dim=0)`), also with autograd through them.  The matrix products of the
// trunk and the streams stay in csrc/dense.hip: they run on the EFFECTIVE parameter vector that noisy_compose_kernel writes in
// tsm_mlp_* layout, and noisy_grad_kernel maps their gradient slabs back onto the net's own flat vector.
//
// Every kernel is elementwise or a fold over at most 64 actions: one element (or one (row, atom) column) per thread, consecutive
// threads on consecutive addresses, f32 throughout, no product fused into a sum (-ffp-contract=off), every sum in action order.
// The layer table travels by value in the kernel arguments; the workgroup's layer is blockIdx.y, so its entry is read with a
// uniform index.
#include "common.h"
#include "philox.h"

namespace {

constexpr int kRThreads = 256;
constexpr int kRMaxDim = 65536;
constexpr int64_t kRMaxRows = (int64_t)1 << 31;
constexpr uint64_t kNoiseKey = 0x52424E4F4953455Full;   // folded into the seed: a Philox key no other draw uses

__device__ __forceinline__ int64_t layer_w(const tsm_noisy_layer &L) { return (int64_t)L.n_in * L.n_out; }

// ---- tsm_noisy_sample ------------------------------------------------------------------------------------------------
// One thread per Philox block = four consecutive slots.  The slots of a layer are contiguous in the flat vector (eps_p [in]
// then eps_q [out] behind the four trained blocks), so slot s of layer l lives at off + 2 in out + 2 out + (s - slot_off).
__device__ __forceinline__ void box_muller(uint32_t wa, uint32_t wb, float &z0, float &z1) {
    const float u1 = (float)((wa >> 8) + 1u) * (1.0f / 16777216.0f);   // (0, 1]: the logarithm never sees 0
    const float u2 = tsm_u01(wb);
    const float r = sqrtf(-2.0f * logf(u1));
    const float t = 6.28318530717958647692f * u2;
    z0 = r * cosf(t);
    z1 = r * sinf(t);
}

__device__ __forceinline__ float noisy_f(float x) {   // discrete.py:360
    const float g = sqrtf(fabsf(x));
    return x < 0.f ? -g : (x > 0.f ? g : 0.f);
}

__global__ __launch_bounds__(kRThreads) void noisy_sample_kernel(tsm_noisy_net net, float *__restrict__ flat, uint64_t seed,
                                                                 uint64_t offset, const uint64_t *__restrict__ offset_dev) {
    const int64_t blk = (int64_t)blockIdx.x * kRThreads + threadIdx.x;
    if (blk * 4 >= net.n_slots) return;
    const uint64_t counter = offset + (offset_dev ? *offset_dev : 0ull);
    uint32_t w[4];
    tsm_philox4_sub(seed ^ kNoiseKey, counter, (uint32_t)blk, w);
    float z[4];
    box_muller(w[0], w[1], z[0], z[1]);
    box_muller(w[2], w[3], z[2], z[3]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t s = blk * 4 + j;
        if (s >= net.n_slots) break;
        int64_t addr = -1;
        for (int l = 0; l < net.n_layers; ++l) {
            const tsm_noisy_layer L = net.layer[l];
            const int64_t k = s - L.slot_off;
            if (L.noisy && k >= 0 && k < (int64_t)L.n_in + L.n_out) addr = L.off + 2 * layer_w(L) + 2 * (int64_t)L.n_out + k;
        }
        if (addr >= 0) flat[addr] = noisy_f(z[j]);
    }
}

// ---- tsm_noisy_compose -----------------------------------------------------------------------------------------------
// grid (ceil(largest layer / 256), n_layers): thread j of layer l writes effective element j (W row-major, then b).
__global__ __launch_bounds__(kRThreads) void noisy_compose_kernel(tsm_noisy_net net, const float *__restrict__ flat,
                                                                  int training, float *__restrict__ eff) {
    const tsm_noisy_layer L = net.layer[blockIdx.y];
    const int64_t nw = layer_w(L), j = (int64_t)blockIdx.x * kRThreads + threadIdx.x;
    if (j >= nw + L.n_out) return;
    const float *p = flat + L.off;
    float val;
    if (!L.noisy) {
        val = p[j];
    } else {
        const float *eps_p = p + 2 * nw + 2 * (int64_t)L.n_out, *eps_q = eps_p + L.n_in;
        if (j < nw) {
            val = p[j];
            if (training) {
                const int o = (int)(j / L.n_in), i = (int)(j - (int64_t)o * L.n_in);
                const float e = eps_q[o] * eps_p[i];   // the outer product first (discrete.py:369)
                val = val + p[nw + j] * e;
            }
        } else {
            const int o = (int)(j - nw);
            val = p[2 * nw + o];
            if (training) val = val + p[2 * nw + L.n_out + o] * eps_q[o];
        }
    }
    eff[L.eff_off + j] = val;
}

// ---- tsm_noisy_grad --------------------------------------------------------------------------------------------------
// grid (ceil(largest layer / 256), n_layers, n_split): thread j of layer l in slab z maps effective gradient j; the first
// in + out threads of a noisy layer (in + out <= in out + out) also clear its noise slots.
__global__ __launch_bounds__(kRThreads) void noisy_grad_kernel(tsm_noisy_net net, const float *__restrict__ flat,
                                                               const float *__restrict__ eff_slabs, int training,
                                                               float *__restrict__ slabs) {
    const tsm_noisy_layer L = net.layer[blockIdx.y];
    const int64_t nw = layer_w(L), j = (int64_t)blockIdx.x * kRThreads + threadIdx.x;
    if (j >= nw + L.n_out) return;
    const float g = eff_slabs[(int64_t)blockIdx.z * net.P_eff + L.eff_off + j];
    float *d = slabs + (int64_t)blockIdx.z * net.P + L.off;
    if (!L.noisy) {
        d[j] = g;
        return;
    }
    const float *eps_p = flat + L.off + 2 * nw + 2 * (int64_t)L.n_out, *eps_q = eps_p + L.n_in;
    if (j < nw) {
        const int o = (int)(j / L.n_in), i = (int)(j - (int64_t)o * L.n_in);
        d[j] = g;
        d[nw + j] = training ? g * (eps_q[o] * eps_p[i]) : 0.f;
    } else {
        const int o = (int)(j - nw);
        d[2 * nw + o] = g;
        d[2 * nw + L.n_out + o] = training ? g * eps_q[o] : 0.f;
    }
    if (j < (int64_t)L.n_in + L.n_out) d[2 * nw + 2 * (int64_t)L.n_out + j] = 0.f;
}

// ---- dueling streams ---------------------------------------------------------------------------------------------------
// One thread per (row, atom): the n_act values of a column are n_atoms floats apart, consecutive threads read consecutive atoms.
__global__ __launch_bounds__(kRThreads) void dueling_combine_kernel(const float *__restrict__ q, const float *__restrict__ v,
                                                                    int64_t R, int32_t A, int32_t N, float *__restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * kRThreads + threadIdx.x;
    if (t >= R * N) return;
    const int64_t r = t / N;
    const int n = (int)(t - r * N);
    const float *qc = q + r * A * N + n;
    float s = 0.f;
    for (int a = 0; a < A; ++a) s += qc[(int64_t)a * N];
    const float mean = s / (float)A, vv = v[t];
    float *oc = out + r * A * N + n;
    for (int a = 0; a < A; ++a) oc[(int64_t)a * N] = (qc[(int64_t)a * N] - mean) + vv;
}

__global__ __launch_bounds__(kRThreads) void dueling_combine_backward_kernel(const float *__restrict__ d, int64_t R, int32_t A,
                                                                             int32_t N, float *__restrict__ d_q,
                                                                             float *__restrict__ d_v) {
    const int64_t t = (int64_t)blockIdx.x * kRThreads + threadIdx.x;
    if (t >= R * N) return;
    const int64_t r = t / N;
    const int n = (int)(t - r * N);
    const float *dc = d + r * A * N + n;
    float s = 0.f;
    for (int a = 0; a < A; ++a) s += dc[(int64_t)a * N];
    const float m = s / (float)A;
    float *qc = d_q + r * A * N + n;
    for (int a = 0; a < A; ++a) qc[(int64_t)a * N] = dc[(int64_t)a * N] - m;
    d_v[t] = s;
}

__global__ __launch_bounds__(kRThreads) void dueling_features_kernel(const float *__restrict__ z, int64_t n, float *__restrict__ f) {
    const int64_t t = (int64_t)blockIdx.x * kRThreads + threadIdx.x;
    if (t < n) f[t] = fmaxf(z[t], 0.f);
}

__global__ __launch_bounds__(kRThreads) void dueling_features_backward_kernel(const float *__restrict__ z,
                                                                              const float *__restrict__ d_fq,
                                                                              const float *__restrict__ d_fv, int64_t n,
                                                                              float *__restrict__ d_z) {
    const int64_t t = (int64_t)blockIdx.x * kRThreads + threadIdx.x;
    if (t < n) d_z[t] = z[t] > 0.f ? d_fq[t] + d_fv[t] : 0.f;
}

int net_check(const char *who, const tsm_noisy_net *net) {
    TSM_REQUIRE(net, "%s: null layer table", who);
    TSM_REQUIRE(net->n_layers >= 1 && net->n_layers <= TSM_NOISY_MAX_LAYERS, "%s: n_layers = %d outside [1, %d]", who,
                net->n_layers, TSM_NOISY_MAX_LAYERS);
    int64_t off = 0, eff = 0, slot = 0;
    for (int l = 0; l < net->n_layers; ++l) {
        const tsm_noisy_layer &L = net->layer[l];
        TSM_REQUIRE(L.n_in >= 1 && L.n_in <= kRMaxDim && L.n_out >= 1 && L.n_out <= kRMaxDim,
                    "%s: layer %d is %d -> %d, widths must lie in [1, %d]", who, l, L.n_in, L.n_out, kRMaxDim);
        TSM_REQUIRE(L.noisy == 0 || L.noisy == 1, "%s: layer %d: noisy = %d is neither 0 nor 1", who, l, L.noisy);
        TSM_REQUIRE(L.off == off && L.eff_off == eff && L.slot_off == slot,
                    "%s: layer %d starts at (%lld, %lld, slot %lld), the layers before it end at (%lld, %lld, slot %lld)", who, l,
                    (long long)L.off, (long long)L.eff_off, (long long)L.slot_off, (long long)off, (long long)eff, (long long)slot);
        const int64_t nw = (int64_t)L.n_in * L.n_out;
        off += L.noisy ? 2 * nw + 3 * (int64_t)L.n_out + L.n_in : nw + L.n_out;
        eff += nw + L.n_out;
        slot += L.noisy ? (int64_t)L.n_in + L.n_out : 0;
    }
    TSM_REQUIRE(net->P == off && net->P_eff == eff && net->n_slots == slot,
                "%s: the table says P = %lld, P_eff = %lld, n_slots = %lld, its layers add up to %lld, %lld, %lld", who,
                (long long)net->P, (long long)net->P_eff, (long long)net->n_slots, (long long)off, (long long)eff, (long long)slot);
    TSM_REQUIRE(off < ((int64_t)1 << 31), "%s: P = %lld does not fit 31 bits", who, (long long)off);
    return TSM_OK;
}

int64_t largest_layer(const tsm_noisy_net *net) {
    int64_t m = 0;
    for (int l = 0; l < net->n_layers; ++l) {
        const int64_t n = (int64_t)net->layer[l].n_in * net->layer[l].n_out + net->layer[l].n_out;
        m = n > m ? n : m;
    }
    return m;
}

int dueling_check(const char *who, int64_t R, int32_t n_act, int32_t n_atoms) {
    if (int rc = tsm_distq_check(n_act, n_atoms)) return rc;
    TSM_REQUIRE(R >= 0 && R * n_act * n_atoms < kRMaxRows, "%s: R = %lld out of range", who, (long long)R);
    return TSM_OK;
}

}  // namespace

TSM_EXPORT int tsm_rainbow_check(const tsm_noisy_net *net) { return net_check("tsm_rainbow_check", net); }

TSM_EXPORT int tsm_noisy_sample(const tsm_noisy_net *net, float *flat, uint64_t seed, uint64_t offset,
                                const uint64_t *offset_dev, void *stream) {
    if (int rc = net_check("tsm_noisy_sample", net)) return rc;
    if (net->n_slots == 0) return TSM_OK;
    TSM_REQUIRE(flat, "tsm_noisy_sample: null pointer");
    const int64_t blocks = ceil_div(net->n_slots, 4);
    hipLaunchKernelGGL(noisy_sample_kernel, dim3((unsigned)ceil_div(blocks, kRThreads)), dim3(kRThreads), 0, tsm_stream(stream),
                       *net, flat, seed, offset, offset_dev);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_noisy_compose(const tsm_noisy_net *net, const float *flat, int training, float *eff, void *stream) {
    if (int rc = net_check("tsm_noisy_compose", net)) return rc;
    TSM_REQUIRE(flat && eff, "tsm_noisy_compose: null pointer");
    hipLaunchKernelGGL(noisy_compose_kernel, dim3((unsigned)ceil_div(largest_layer(net), kRThreads), (unsigned)net->n_layers),
                       dim3(kRThreads), 0, tsm_stream(stream), *net, flat, training, eff);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_noisy_grad(const tsm_noisy_net *net, const float *flat, const float *eff_slabs, int32_t n_split, int training,
                              float *slabs, void *stream) {
    if (int rc = net_check("tsm_noisy_grad", net)) return rc;
    TSM_REQUIRE(n_split >= 1 && n_split <= 65535, "tsm_noisy_grad: n_split = %d outside [1, 65535]", n_split);
    TSM_REQUIRE(flat && eff_slabs && slabs, "tsm_noisy_grad: null pointer");
    hipLaunchKernelGGL(noisy_grad_kernel,
                       dim3((unsigned)ceil_div(largest_layer(net), kRThreads), (unsigned)net->n_layers, (unsigned)n_split),
                       dim3(kRThreads), 0, tsm_stream(stream), *net, flat, eff_slabs, training, slabs);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_dueling_combine(const float *q, const float *v, int64_t R, int32_t n_act, int32_t n_atoms, float *out,
                                   void *stream) {
    if (int rc = dueling_check("tsm_dueling_combine", R, n_act, n_atoms)) return rc;
    if (R == 0) return TSM_OK;
    TSM_REQUIRE(q && v && out, "tsm_dueling_combine: null pointer");
    hipLaunchKernelGGL(dueling_combine_kernel, dim3((unsigned)ceil_div(R * n_atoms, kRThreads)), dim3(kRThreads), 0,
                       tsm_stream(stream), q, v, R, n_act, n_atoms, out);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_dueling_combine_backward(const float *d, int64_t R, int32_t n_act, int32_t n_atoms, float *d_q, float *d_v,
                                            void *stream) {
    if (int rc = dueling_check("tsm_dueling_combine_backward", R, n_act, n_atoms)) return rc;
    if (R == 0) return TSM_OK;
    TSM_REQUIRE(d && d_q && d_v, "tsm_dueling_combine_backward: null pointer");
    hipLaunchKernelGGL(dueling_combine_backward_kernel, dim3((unsigned)ceil_div(R * n_atoms, kRThreads)), dim3(kRThreads), 0,
                       tsm_stream(stream), d, R, n_act, n_atoms, d_q, d_v);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_dueling_features(const float *z, int64_t n, float *f, void *stream) {
    TSM_REQUIRE(n >= 0 && n < kRMaxRows, "tsm_dueling_features: n = %lld out of range", (long long)n);
    if (n == 0) return TSM_OK;
    TSM_REQUIRE(z && f, "tsm_dueling_features: null pointer");
    hipLaunchKernelGGL(dueling_features_kernel, dim3((unsigned)ceil_div(n, kRThreads)), dim3(kRThreads), 0, tsm_stream(stream), z,
                       n, f);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}

TSM_EXPORT int tsm_dueling_features_backward(const float *z, const float *d_fq, const float *d_fv, int64_t n, float *d_z,
                                             void *stream) {
    TSM_REQUIRE(n >= 0 && n < kRMaxRows, "tsm_dueling_features_backward: n = %lld out of range", (long long)n);
    if (n == 0) return TSM_OK;
    TSM_REQUIRE(z && d_fq && d_fv && d_z, "tsm_dueling_features_backward: null pointer");
    hipLaunchKernelGGL(dueling_features_backward_kernel, dim3((unsigned)ceil_div(n, kRThreads)), dim3(kRThreads), 0,
                       tsm_stream(stream), z, d_fq, d_fv, n, d_z);
    TSM_LAUNCH_CHECK();
    return TSM_OK;
}
