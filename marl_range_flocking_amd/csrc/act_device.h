// Device helpers shared by the fused acting kernels (flock_vdn_act.hip, whose header tells the layout they assume, and
// flock_maddpg_act.hip): lane (j, g) = (lane & 15, lane >> 4) holds elements 16 T + 4 g + v (v = 0..3) of row j for
// every 16-wide tile T of an activation. Include after `#pragma clang fp contract(off)`.
#pragma once

#include "learn_device.h"

namespace flock_act_device {
using namespace flock_learn_device;

constexpr int kBlock = 256, kH = 32, kG = 3 * kH;  // 4 waves; the hidden width; gate rows (r, z, n)
static_assert(kG == kFG && kH == kF2, "the acting kernels share the QNet's GRU shape");

// Column swizzle of a weight row o (o & 15 = i) that is staged unpadded: element (o, k) lies at o * K + (k ^ swz(i)),
// bits 0, 1 <- i bits 0, 1; bit 3 <- i bit 2; bit 4 <- i bit 3, so the 32 lanes of a half-wave (16 weight rows x 2
// lane groups, whose k differ in bit 2) read 32 distinct banks.
__device__ __forceinline__ int swz(int i) { return (i & 3) | ((i & 4) << 1) | ((i & 8) << 1); }

// acc[T] += W[16 T + i][k] * act[k][row], one MFMA per tile: `wk` points at this lane's (i, k) element of tile 0
template <int NT, int K>
__device__ __forceinline__ void mfma_wt(f32x4_t (&acc)[NT], const float* wk, float act) {
#pragma unroll
    for (int T = 0; T < NT; ++T) acc[T] = __builtin_amdgcn_mfma_f32_16x16x4f32(wk[16 * T * K], act, acc[T], 0, 0, 0);
}

// Row split: agent a's B rows, in tiles of `rows`, go to S blocks in contiguous runs. Work item w = a * S + s runs on
// block b with w = xcd_first(b % 8) + b / 8 (the items of one XCD label b % 8 are consecutive; a bijection for any grid
// of A * S blocks), so the blocks reading one agent's weights, and neighbouring agents whose observations share cache
// lines, share an XCD's L2. Placement changes speed only: no block reads what another writes. An empty run leaves.
struct RowRun { int64_t a, r_begin, r_end; };
__device__ __forceinline__ RowRun row_run(int A, int S, int B, int rows) {
    const int Wn = A * S, bx = blockIdx.x, q8 = Wn >> 3, r8 = Wn & 7, xl = bx & 7;
    const int w = (xl < r8 ? xl * (q8 + 1) : r8 * (q8 + 1) + (xl - r8) * q8) + (bx >> 3);
    const int64_t a = w / S;
    const int s = w - (int)a * S;
    const int tiles = (B + rows - 1) / rows, tps = (tiles + S - 1) / S;
    const int64_t r_begin = (int64_t)s * tps * rows;
    return {a, r_begin, min((int64_t)B, r_begin + (int64_t)tps * rows)};
}

// Staging of agent a's matrix out of the stacked weights W [A, out, K]. A small-input matrix (K <= 16): row pitch
// K1 + 2 = 2 (2 u + 1), so 16 rows x 2 adjacent k fall on 32 distinct banks; columns K .. K1 - 1 (K1 = K up to 4) zero.
__device__ __forceinline__ void stage_small_in(float* dst, const float* W, int64_t a, int out, int K, int tid) {
    const int K1 = (K + 3) & ~3, sx = K1 + 2;
    for (int e = tid; e < out * K1; e += kBlock) {
        const int o = e / K1, k = e - o * K1;
        dst[o * sx + k] = k < K ? W[(a * out + o) * K + k] : 0.0f;
    }
}

// The two GRU gate matrices weight_ih, weight_hh [A, kG, kH], swizzled
__device__ __forceinline__ void stage_gates(float* wi, float* wh, const float* Wi, const float* Wh, int64_t a,
                                            int tid) {
    for (int e = tid; e < kG * kH; e += kBlock) {
        const int o = e / kH, k = e % kH, d = o * kH + (k ^ swz(o & 15));
        wi[d] = Wi[a * kG * kH + e];
        wh[d] = Wh[a * kG * kH + e];
    }
}

// The small-input layer on NT feature tiles: acc[T] += W[16 T + j][k] x[k] with k = 4 s + g from lane group g.
// `wl` = the staged matrix (stage_small_in) + j * (K1 + 2) + g; x[s] = this lane's input element 4 s + g.
template <int NT>
__device__ __forceinline__ void small_in_layer(f32x4_t (&acc)[NT], const float* wl, int K1,
                                               const float (&x)[kFMaxIn / 4]) {
    const int sx = K1 + 2;
#pragma unroll
    for (int s4 = 0; s4 < kFMaxIn / 4; ++s4)
        if (4 * s4 < K1) {
            const float xs = x[s4];
            const float* ws = wl + 4 * s4;
#pragma unroll
            for (int T = 0; T < NT; ++T)
                acc[T] = __builtin_amdgcn_mfma_f32_16x16x4f32(ws[16 * T * sx], xs, acc[T], 0, 0, 0);
        }
}

// ho = GRUCell(y, h): both gate products (12 tiles; MFMA (T', v) takes k = 16 T' + 4 g + v, the order the lanes hold y
// and h, so r, z, n of hidden column c sit in one lane and slot of tiles t, t + 2, t + 4) and the cell on the
// accumulators, in gru_fwd_kernel's operation order. wil / whl: the staged gate matrices + j * kH; bsi / bsh: bias_ih /
// bias_hh [kG] in LDS; m = (4 g) ^ swz(j).
__device__ __forceinline__ void gru_step(float (&ho)[2][4], const float (&y)[2][4], const float (&h)[2][4],
                                         const float* wil, const float* whl, const float* bsi, const float* bsh,
                                         int m, int g) {
    f32x4_t gi[6] = {}, gh[6] = {};
#pragma unroll
    for (int Tp = 0; Tp < 2; ++Tp)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int c = (16 * Tp + v) ^ m;
            mfma_wt<6, kH>(gi, wil + c, y[Tp][v]);
            mfma_wt<6, kH>(gh, whl + c, h[Tp][v]);
        }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int c = 16 * t + 4 * g + v;
            const float air = gi[t][v] + bsi[c], aiz = gi[t + 2][v] + bsi[kH + c], ain = gi[t + 4][v] + bsi[2 * kH + c];
            const float bhr = gh[t][v] + bsh[c], bhz = gh[t + 2][v] + bsh[kH + c], ghn = gh[t + 4][v] + bsh[2 * kH + c];
            const float rg = sigmoidf_(bhr + air);
            const float zg = sigmoidf_(bhz + aiz);
            const float nn = tanhf(ain + ghn * rg);
            ho[t][v] = (h[t][v] - nn) * zg + nn;
        }
}

// A row's hidden state as the lanes hold it: two 16-B accesses at hp = the row + 4 g, the four lanes of a row cover
// its 128 B. `zero`: the row's reset flag (it may come with the load), h = 0 for a row that starts an episode.
__device__ __forceinline__ void load_h(float4 (&hr)[2], const float* hp) {
    hr[0] = *reinterpret_cast<const float4*>(hp);
    hr[1] = *reinterpret_cast<const float4*>(hp + 16);
}
__device__ __forceinline__ void unpack_h(float (&h)[2][4], const float4 (&hr)[2], bool zero) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
        h[t][0] = zero ? 0.0f : hr[t].x, h[t][1] = zero ? 0.0f : hr[t].y, h[t][2] = zero ? 0.0f : hr[t].z,
        h[t][3] = zero ? 0.0f : hr[t].w;
}
__device__ __forceinline__ void store_h(float* hp, const float (&ho)[2][4]) {
    *reinterpret_cast<float4*>(hp) = make_float4(ho[0][0], ho[0][1], ho[0][2], ho[0][3]);
    *reinterpret_cast<float4*>(hp + 16) = make_float4(ho[1][0], ho[1][1], ho[1][2], ho[1][3]);
}

}  // namespace flock_act_device
