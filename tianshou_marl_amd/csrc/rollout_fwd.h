// rollout_fwd.h -- the eight-wave tile forward of rollout.hip with the launch's constants taken off the per-step chain.
//
// tile_forward_split (mlp_tile.h) is written for one forward per launch: every call re-reads its weight fragments, biases and the
// critic's W3 vector from LDS behind each barrier, and reads the activation operand as 16 four-float-strided scalars per lane and layer.
// The persistent rollout calls it 27 times per collect with a frozen policy, and a wave owns the same 16-column block of the same net in
// every call.  Here
//   * FwdRegs holds a wave's fragments in registers for the whole launch (loaded once behind the staging barrier), and
//   * H1 / H2 are kept k-fragment-major (hk_off below): the 16 activations a lane feeds to its 16 MFMAs of a layer are contiguous, four
//     16-byte LDS reads instead of sixteen 4-byte ones.
// The MFMAs, their operands and their order are tile_forward_split's, the critic's value is the same fmaf chain j = 0 .. H - 1:
// bit-identical outputs (tests/test_gpu_rollout_regs.py).  OUT (logits | value) keeps Lay<H>'s layout; H1 / H2 in the new layout are
// private to this forward (each net's block is 16 x 64 floats inside the R x ld2 floats Lay<H> reserves: nothing else moves).
#pragma once
#include "mlp_tile.h"

namespace {

// Offset (floats, inside one net's 1024-float block) of activation (tile row, hidden column c = 4 kb + kq).
//   address bits [9:8] = kq         the k-lane that reads it (the block of a k-lane is 256 floats: neutral for every bank rule)
//                [7:4] = row bits (b3, b1, b0, b2)
//                [3:2] = (kb >> 2) ^ kq ^ (b3, b1)      the 16-byte chunk, swizzled
//                [1:0] = kb & 3
// Reads (ds_read_b128, lane = (row r16, k-lane kq), chunk q = 0 .. 3; banks are address mod 64 floats, i.e. 16 slots of 16 bytes, and
// conflict inside the instruction's four 16-lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32): a group holds
// every row once, with kq = 2 h + (b2 ^ b3) or 2 h + 1 - (b2 ^ b3).  The slot is (b0, b2 | q ^ kq ^ (b3, b1)): among the four rows that
// share (b0, b2) the chunk bits are (b3 ^ h, b1 ^ b2 ^ b3 [^ 1]) ^ q -- four different chunks, so the 16 lanes of a group read 16 different
// slots: conflict-free.  The value lanes (one per row, all chunks of all k-lanes) see the same rule with kq fixed.
// Writes (ds_write_b32 of the epilogue, banks = address mod 32 within a 32-lane half: lane (column r16 of the wave's block w, rows
// 4 kq + r) -> kq' = r16 & 3, kb = 4 w + (r16 >> 2)): bank = (b2 | w ^ kq' ^ (b3, b1) | r16 >> 2) with b2 = kq & 1 and b3, b1 fixed in a
// half: 2 x 4 x 4 = 32 different banks, conflict-free as well (the row-major layout wrote two-way).
__device__ __forceinline__ int hk_row(int row) {   // the row's part of the offset
    return ((row & 8) | ((row & 3) << 1) | ((row >> 2) & 1)) << 4;
}
__device__ __forceinline__ int hk_swz(int row, int kq) {   // the chunk swizzle of (row, k-lane), as a float offset 0 / 4 / 8 / 12
    return ((kq ^ ((row >> 2) & 2) ^ ((row >> 1) & 1)) & 3) << 2;
}
__device__ __forceinline__ int hk_off(int row, int c) {
    const int kq = c & 3, kb = c >> 2;
    return kq * 256 + hk_row(row) + (((kb >> 2) << 2) ^ hk_swz(row, kq)) + (kb & 3);
}

// A wave's launch constants.  KB1: k-steps of layer 1 the registers hold: Kp1 / 4 when the observation width is a compile-time value,
// else 0 -- the generic instantiation keeps W1 in LDS (16 more registers for its worst case spilled five of them).  w3: wave 0's W3a fragment; b3: its bias on wave 0, the critic's on wave 5.  (The value lanes' W3 vector is NOT
// here: 64 more registers on every wave put the kernel, 191-198 registers before, into scratch -- it is read 16 bytes at a time instead.)
template <int H, int KB1>
struct FwdRegs {
    float w1[KB1 ? KB1 : 1], w2[H / 4], w3[H / 4], b1, b2, b3;
};

template <int H, int KB1>
__device__ __forceinline__ void fwd_regs_load(FwdRegs<H, KB1> &g, const float *lds, const Lay<H> &ly, const Dims &d) {
    const int lane = threadIdx.x & 63, w8 = threadIdx.x >> 6, net = w8 >> 2, w = w8 & 3;
    const int r16 = lane & 15, kq = lane >> 4;
    const int col = 16 * w + r16;
    const float *w1p = lds + ly.W1 + (net * H + col) * d.ld1 + kq;
    const float *w2p = lds + (net ? ly.W2c : ly.W2a) + col * ly.ldh + kq;
#pragma unroll
    for (int kb = 0; kb < KB1; ++kb) g.w1[kb] = w1p[4 * kb];
#pragma unroll
    for (int kb = 0; kb < H / 4; ++kb) g.w2[kb] = w2p[4 * kb];
    g.b1 = lds[ly.B1 + net * H + col];
    g.b2 = lds[ly.B2 + net * H + col];
#pragma unroll
    for (int kb = 0; kb < H / 4; ++kb) g.w3[kb] = 0.f;
    g.b3 = 0.f;
    if (w8 == 0) {
        const float *w3p = lds + ly.W3a + r16 * ly.ldh + kq;
#pragma unroll
        for (int kb = 0; kb < H / 4; ++kb) g.w3[kb] = w3p[4 * kb];
        g.b3 = lds[ly.B3a + r16];
    } else if (w8 == 5) {
        g.b3 = lds[ly.B3c];
    }
}

// tile_forward_split with the weights from FwdRegs and H1 / H2 k-fragment-major.  All 512 threads call it (three barriers inside).
template <int H, int KB1>
__device__ __forceinline__ void tile_forward_regs(float *lds, const Lay<H> &ly, const Dims &d, const FwdRegs<H, KB1> &g) {
    static_assert(H == 64 && 2 * 16 * H <= R * Lay<H>::ld2, "hk_off: two 16 x 64 blocks inside an activation buffer");
    constexpr int KBH = H / 4;
    const int lane = threadIdx.x & 63, w8 = threadIdx.x >> 6, net = w8 >> 2, w = w8 & 3;
    const int r16 = lane & 15, kq = lane >> 4;
    const int col = 16 * w + r16;
    // a lane's 16 activations of a layer, in k order, from buffer `buf` (H1 or H2) of net `n`
    auto act_frags = [&](int buf, int n, float (&a)[KBH]) {
        const float *base = lds + buf + n * (16 * H) + kq * 256 + hk_row(r16);
        const int sw = hk_swz(r16, kq);
#pragma unroll
        for (int q = 0; q < KBH / 4; ++q) {
            const f4 v = *reinterpret_cast<const f4 *>(base + ((4 * q) ^ sw));
            a[4 * q] = v[0]; a[4 * q + 1] = v[1]; a[4 * q + 2] = v[2]; a[4 * q + 3] = v[3];
        }
    };
    // epilogue of a hidden layer: bias + ReLU of rows 4 kq + r, column col of net `net`
    auto put = [&](int buf, const f4 &acc, float b) {
#pragma unroll
        for (int r = 0; r < 4; ++r) lds[buf + net * (16 * H) + hk_off(kq * 4 + r, col)] = fmaxf(acc[r] + b, 0.f);
    };
    {   // L1
        f4 acc = {0.f, 0.f, 0.f, 0.f};
        const float *xa = lds + ly.X + r16 * d.ld1 + kq;
        if constexpr (KB1 > 0) {
#pragma unroll
            for (int kb = 0; kb < KB1; ++kb) acc = mfma(xa[4 * kb], g.w1[kb], acc);
        } else {
            const float *wp = lds + ly.W1 + (net * H + col) * d.ld1 + kq;
            for (int k0 = 0; k0 < d.Kp1; k0 += 4) acc = mfma(xa[k0], wp[k0], acc);
        }
        put(ly.H1, acc, g.b1);
    }
    __syncthreads();
    {   // L2
        f4 acc = {0.f, 0.f, 0.f, 0.f};
        float a[KBH];
        act_frags(ly.H1, net, a);
#pragma unroll
        for (int kb = 0; kb < KBH; ++kb) acc = mfma(a[kb], g.w2[kb], acc);
        put(ly.H2, acc, g.b2);
    }
    __syncthreads();
    if (w8 == 0) {  // logits (MFMA, A padded to 16)
        f4 acc = {0.f, 0.f, 0.f, 0.f};
        float a[KBH];
        act_frags(ly.H2, 0, a);
#pragma unroll
        for (int kb = 0; kb < KBH; ++kb) acc = mfma(a[kb], g.w3[kb], acc);
#pragma unroll
        for (int r = 0; r < 4; ++r) lds[ly.OUT + (kq * 4 + r) * ly.ldo + r16] = acc[r] + g.b3;
    } else if (w8 == 5 && lane < R) {  // value (VALU dot) on wave 5, as in tile_forward_split: s = fmaf(h[j], w3[j], s), j = 0 .. H - 1,
        // 16 steps of the chain at a time: chunk q of every k-lane's block holds h[16 q + 4 i + k]; W3c as four 16-byte words
        float s = 0.f;
        const float *base = lds + ly.H2 + 16 * H + hk_row(lane);
#pragma unroll
        for (int q = 0; q < KBH / 4; ++q) {
            f4 hv[4], wv[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                hv[k] = *reinterpret_cast<const f4 *>(base + k * 256 + ((4 * q) ^ hk_swz(lane, k)));
                wv[k] = *reinterpret_cast<const f4 *>(lds + ly.W3c + 16 * q + 4 * k);
            }
#pragma unroll
            for (int j = 0; j < 16; ++j) s = fmaf(hv[j & 3][j >> 2], wv[j >> 2][j & 3], s);
        }
        lds[ly.OUT + lane * ly.ldo + 16] = s + g.b3;
    }
    __syncthreads();
}

}  // namespace
