// flock_vdn_act.hip — the acting step of the recurrent VDN QNet for every (env row, agent) in ONE launch (gfx950).
//
// QNet.sample_action (learners/vdn/net.py:27-37, :52-58) per row b and agent a, with agent a's own weights:
//   y1 = relu(W1 x + b1) [64]   y2 = relu(W2 y1 + b2) [32]
//   gi = Wih y2 + bih, gh = Whh h + bhh [96 each, gates r, z, n]
//   r = sigmoid(gh_r + gi_r)  z = sigmoid(gh_z + gi_z)  n = tanh(gi_n + gh_n r)  h' = (h - n) z + n   (gru_fwd_kernel)
//   q = Wq h' + bq [n_actions]   action = coin[b] <= epsilon ? rnd[b][a] : argmax_j q[j] (lowest j among equal maxima)
// The torch chain it replaces (BatchedQNet.forward_am + argmax + where) runs four batched GEMMs, two ReLU passes, the
// GRU gate kernel and two transposes, every intermediate through HBM; here a row moves its observation, its hidden
// state in and out and one action id.
//
// Layout. A block of 4 waves stages ONE agent's weights in LDS once and walks a run of that agent's row tiles (64
// rows); wave w takes rows [16 w, 16 w + 16) of each tile and shares nothing else with the other waves: after the
// weights' barrier there is no barrier and no activation in LDS. Every layer is f32 MFMA (v_mfma_f32_16x16x4_f32:
// each output a k-ordered fmaf chain) computed TRANSPOSED, out^T = W act^T: the A operand is a weight tile (16 output
// features x 4 k, from LDS), the B operand the activations (4 k x 16 rows), the result D[feature][row]. Lane (j, g) =
// (lane & 15, lane >> 4) then holds, for every 16-feature tile T of a layer's output, features 16 T + 4 g + v
// (v = 0..3) of row j — and a B operand wants from lane (j, g) one activation of row j per MFMA, any k the other
// lanes of the MFMA do not supply. So the next layer sums its k in the order the lanes hold them: MFMA (T', v) takes
// k = 16 T' + 4 g + v from lane group g, straight from the accumulators' registers (bias and ReLU applied there).
// The same holds for the hidden state, which each lane loads in that pattern (two 16-B loads: the four lanes of a row
// cover its 128 B), for both gate products (so r, z, n of hidden column c sit in one lane and slot of tiles t, t + 2,
// t + 4 and the GRU cell runs in registers), for h' (stored as it was loaded) and for the q head, whose 16 outputs per
// row lie 4 to a lane: argmax is a scan of those 4 and two xor steps (lanes 16 and 32 apart) carrying (value, index).
// x is loaded by the lane that feeds it to layer 1 (k = 4 s + g). The next 16 rows' x, h, reset flag, coin and random
// id are in flight while the current ones compute. A row's result depends on nothing but that row and the weights:
// not on its place in the tile, the block or the grid.
// LDS (floats): W1 64 x (K1 + 2), W2 32 x 64, Wih 96 x 32, Whh 96 x 32, Wq 16 x 32 (rows >= n_actions zero), biases
// 304: 10160 floats = 40.6 KB. W2 / Wih / Whh / Wq rows are unpadded and XOR-swizzled: element (o, k) at
// o * K + (k ^ sw(o & 15)), sw(i) = bits {0, 1, 3, 4} <- i, so the 32 lanes of a half-wave (16 weight rows x 2 lane
// groups, whose k differ in bit 2) read 32 distinct banks.
// Row split: agent a's row tiles are dealt to `split` blocks in contiguous runs; work item w = a * split + s runs on
// block b with w = xcd_first(b % 8) + b / 8 (sc_act_kernel's order, made bijective for any grid), so the blocks that
// read one agent's weights, and the neighbouring agents whose observations share cache lines in the [B, A, n] layout,
// share an XCD's L2. Placement changes speed only: no block reads what another block writes.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "flock_learn.h"
#include "learn_internal.h"

#pragma clang fp contract(off)

#include "learn_device.h"

namespace {
using flock_learn_internal::fail;
using flock_learn_internal::launched;
using namespace flock_learn_device;

constexpr int kBlock = 256;
constexpr int kH = 32;       // hidden width
constexpr int kMaxAct = 16;  // one q tile
constexpr int kNBias = kF1 + kF2 + 2 * kFG + kMaxAct;
// LDS offsets (floats)
constexpr int oW1 = 0, oW2 = oW1 + kF1 * kSW1, oWi = oW2 + kF2 * kF1, oWh = oWi + kFG * kH, oWq = oWh + kFG * kH,
              oBs = oWq + kMaxAct * kH, kLdsFloats = oBs + kNBias;
static_assert(kLdsFloats * sizeof(float) <= 48 * 1024, "static LDS; three blocks per CU");

struct VdnActArgs {
    int A, B, NI, NA, S;
    const float *W1, *b1, *W2, *b2, *Wi, *Wh, *bi, *bh, *Wq, *bq;
    const float* obs;
    int64_t o_sr, o_sa;
    const float* hin;
    int64_t hi_sr, hi_sa;
    float* hout;
    int64_t ho_sr, ho_sa;
    void* action;
    int64_t a_sr, a_sa;
    float* q;
    int64_t q_sr, q_sa;
    const float* coin;
    const int64_t* rnd;
    const uint8_t* reset;
    float eps;
    int act_i64;
};

// column swizzle of weight row o (o & 15 = i): bits 0, 1 <- i bits 0, 1; bit 3 <- i bit 2; bit 4 <- i bit 3
__device__ __forceinline__ int swz(int i) { return (i & 3) | ((i & 4) << 1) | ((i & 8) << 1); }

// acc[T] += W[16 T + i][k] * act[k][row], one MFMA per tile: `wk` points at this lane's (i, k) element of tile 0
template <int NT, int K>
__device__ __forceinline__ void mfma_wt(f32x4_t (&acc)[NT], const float* wk, float act) {
#pragma unroll
    for (int T = 0; T < NT; ++T) acc[T] = __builtin_amdgcn_mfma_f32_16x16x4f32(wk[16 * T * K], act, acc[T], 0, 0, 0);
}

// three waves per SIMD (at most 168 registers): with 40.6 KB of LDS, three blocks per CU
__global__ __launch_bounds__(kBlock, 3) void vdn_act_kernel(VdnActArgs p) {
    __shared__ __attribute__((aligned(16))) float sm[kLdsFloats];
    float *w1 = sm + oW1, *w2 = sm + oW2, *wi = sm + oWi, *wh = sm + oWh, *wq = sm + oWq, *bs = sm + oBs;
    const float *bs1 = bs, *bs2 = bs + kF1, *bsi = bs2 + kF2, *bsh = bsi + kFG, *bsq = bsh + kFG;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    // work item of this block: the items of one XCD label (b % 8) are consecutive
    const int Wn = p.A * p.S, bx = blockIdx.x, q8 = Wn >> 3, r8 = Wn & 7, xl = bx & 7;
    const int w = (xl < r8 ? xl * (q8 + 1) : r8 * (q8 + 1) + (xl - r8) * q8) + (bx >> 3);
    const int64_t a = w / p.S;
    const int s = w - (int)a * p.S;
    const int tiles = (p.B + kFRows - 1) / kFRows, tps = (tiles + p.S - 1) / p.S;
    const int64_t r_begin = (int64_t)s * tps * kFRows;
    const int64_t r_end = min((int64_t)p.B, r_begin + (int64_t)tps * kFRows);
    if (r_begin >= r_end) return;  // more blocks than row tiles: nothing to do (the whole block leaves)

    const int NI = p.NI, NA = p.NA;
    const int K1 = (NI + 3) & ~3;
    const int sx = K1 + 2;  // w1 row stride: 2 (2 u + 1), so 16 rows x 2 adjacent k fall on 32 distinct banks
    for (int e = tid; e < kF1 * K1; e += kBlock) {
        const int o = e / K1, k = e - o * K1;
        w1[o * sx + k] = k < NI ? p.W1[(a * kF1 + o) * NI + k] : 0.0f;
    }
    for (int e = tid; e < kF2 * kF1; e += kBlock) {
        const int o = e / kF1, k = e % kF1;
        w2[o * kF1 + (k ^ swz(o & 15))] = p.W2[a * kF2 * kF1 + e];
    }
    for (int e = tid; e < kFG * kH; e += kBlock) {
        const int o = e / kH, k = e % kH, d = o * kH + (k ^ swz(o & 15));
        wi[d] = p.Wi[a * kFG * kH + e];
        wh[d] = p.Wh[a * kFG * kH + e];
    }
    for (int e = tid; e < kMaxAct * kH; e += kBlock) {
        const int o = e / kH, k = e % kH;
        wq[o * kH + (k ^ swz(o))] = e < NA * kH ? p.Wq[a * NA * kH + e] : 0.0f;
    }
    if (tid < kF1) bs[tid] = p.b1[a * kF1 + tid];
    if (tid < kF2) bs[kF1 + tid] = p.b2[a * kF2 + tid];
    if (tid < kFG) {
        bs[kF1 + kF2 + tid] = p.bi[a * kFG + tid];
        bs[kF1 + kF2 + kFG + tid] = p.bh[a * kFG + tid];
    }
    if (tid < kMaxAct) bs[kF1 + kF2 + 2 * kFG + tid] = tid < NA ? p.bq[a * NA + tid] : 0.0f;
    __syncthreads();  // the only barrier: from here on the waves share nothing but these weights

    // lane (j, g): row j of the wave's 16, lane group g. As the A operand's lane it is weight row i = j of a tile.
    const int j = lane & 15, g = lane >> 4;
    const int m = (4 * g) ^ swz(j);  // k = c + 4 g of row i sits at column c ^ m (c: bits 0, 1, 4, 5 only)
    const float* w1l = w1 + j * sx + g;
    const float *w2l = w2 + j * kF1, *wil = wi + j * kH, *whl = wh + j * kH, *wql = wq + j * kH;
    const bool explore = p.coin != nullptr;

    // the next 16 rows in registers: x (k = 4 s + g), h (columns 16 t + 4 g .. + 3), the row's reset flag, and in
    // lanes 0..15 the row's coin and random id
    float xr[kFMaxIn / 4];
    float4 hr[2];
    uint8_t rs = 0;
    float cn = 2.0f;
    int64_t rn = 0;
    auto load = [&](int64_t r) {  // r: this lane's row
        const bool ok = r < r_end;
#pragma unroll
        for (int s4 = 0; s4 < kFMaxIn / 4; ++s4) {
            xr[s4] = 0.0f;
            if (ok && 4 * s4 + g < NI) xr[s4] = p.obs[r * p.o_sr + a * p.o_sa + 4 * s4 + g];
        }
        hr[0] = hr[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        rs = 0;
        cn = 2.0f;  // a coin never exceeds 1: rows past the end stay greedy
        rn = 0;
        if (ok) {
            const float* hp = p.hin + r * p.hi_sr + a * p.hi_sa + 4 * g;
            hr[0] = *reinterpret_cast<const float4*>(hp);
            hr[1] = *reinterpret_cast<const float4*>(hp + 16);
            if (p.reset) rs = p.reset[r];
            if (explore && g == 0) {
                cn = p.coin[r];
                rn = p.rnd[r * p.A + a];
            }
        }
    };
    load(r_begin + 16 * wv + j);
    for (int64_t r0 = r_begin + 16 * wv; r0 < r_end; r0 += kFRows) {
        // the weight fragments are the same every iteration: without this the compiler hoists all 140 LDS reads out
        // of the loop into registers (one wave per SIMD, or spills at the budget below)
        asm volatile("" ::: "memory");
        const int64_t r = r0 + j;
        const bool ok = r < r_end;
        // this group's inputs out of the prefetch registers (an episode start reads h = init_hidden() = 0)
        float x[kFMaxIn / 4], h[2][4];
#pragma unroll
        for (int s4 = 0; s4 < kFMaxIn / 4; ++s4) x[s4] = xr[s4];
        const bool z0 = rs != 0;
        h[0][0] = z0 ? 0.0f : hr[0].x, h[0][1] = z0 ? 0.0f : hr[0].y, h[0][2] = z0 ? 0.0f : hr[0].z,
        h[0][3] = z0 ? 0.0f : hr[0].w;
        h[1][0] = z0 ? 0.0f : hr[1].x, h[1][1] = z0 ? 0.0f : hr[1].y, h[1][2] = z0 ? 0.0f : hr[1].z,
        h[1][3] = z0 ? 0.0f : hr[1].w;
        const int exid = (explore && cn <= p.eps) ? (int)rn : -1;  // lanes 0..15: the row's exploration id
        if (r0 + kFRows < r_end) load(r + kFRows);                 // in flight while these rows compute

        float y1[4][4], y2[2][4];
        {  // layer 1: 4 feature tiles, k = 4 s + g
            f32x4_t acc[4] = {};
#pragma unroll
            for (int s4 = 0; s4 < kFMaxIn / 4; ++s4)
                if (4 * s4 < K1) {
#pragma unroll
                    for (int T = 0; T < 4; ++T)
                        acc[T] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1l[16 * T * sx + 4 * s4], x[s4], acc[T], 0, 0, 0);
                }
#pragma unroll
            for (int T = 0; T < 4; ++T)
#pragma unroll
                for (int v = 0; v < 4; ++v) y1[T][v] = fmaxf(acc[T][v] + bs1[16 * T + 4 * g + v], 0.0f);
        }
        {  // layer 2: 2 feature tiles, k = 16 T' + 4 g + v in the order the lanes hold y1
            f32x4_t acc[2] = {};
#pragma unroll
            for (int Tp = 0; Tp < 4; ++Tp)
#pragma unroll
                for (int v = 0; v < 4; ++v) mfma_wt<2, kF1>(acc, w2l + ((16 * Tp + v) ^ m), y1[Tp][v]);
#pragma unroll
            for (int T = 0; T < 2; ++T)
#pragma unroll
                for (int v = 0; v < 4; ++v) y2[T][v] = fmaxf(acc[T][v] + bs2[16 * T + 4 * g + v], 0.0f);
        }
        float ho[2][4];
        {  // both gate products (12 tiles) and the GRU cell on the accumulators, in gru_fwd_kernel's operation order
            f32x4_t gi[6] = {}, gh[6] = {};
#pragma unroll
            for (int Tp = 0; Tp < 2; ++Tp)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int c = (16 * Tp + v) ^ m;
                    mfma_wt<6, kH>(gi, wil + c, y2[Tp][v]);
                    mfma_wt<6, kH>(gh, whl + c, h[Tp][v]);
                }
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int c = 16 * t + 4 * g + v;
                    const float air = gi[t][v] + bsi[c], aiz = gi[t + 2][v] + bsi[kH + c],
                                ain = gi[t + 4][v] + bsi[2 * kH + c];
                    const float bhr = gh[t][v] + bsh[c], bhz = gh[t + 2][v] + bsh[kH + c],
                                ghn = gh[t + 4][v] + bsh[2 * kH + c];
                    const float rg = sigmoidf_(bhr + air);
                    const float zg = sigmoidf_(bhz + aiz);
                    const float nn = tanhf(ain + ghn * rg);
                    ho[t][v] = (h[t][v] - nn) * zg + nn;
                }
        }
        if (ok) {  // h' as h was loaded: 16 B per lane, the four lanes of a row cover its 128 B
            float* hp = p.hout + r * p.ho_sr + a * p.ho_sa + 4 * g;
            *reinterpret_cast<float4*>(hp) = make_float4(ho[0][0], ho[0][1], ho[0][2], ho[0][3]);
            *reinterpret_cast<float4*>(hp + 16) = make_float4(ho[1][0], ho[1][1], ho[1][2], ho[1][3]);
        }
        {  // q head (this lane: actions 4 g + v of row j) and the action
            f32x4_t qa[1] = {};
#pragma unroll
            for (int Tp = 0; Tp < 2; ++Tp)
#pragma unroll
                for (int v = 0; v < 4; ++v) mfma_wt<1, kH>(qa, wql + ((16 * Tp + v) ^ m), ho[Tp][v]);
            float best = -INFINITY;
            int arg = 4 * g;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int act = 4 * g + v;
                const float qv = qa[0][v] + bsq[act];
                if (p.q && ok && act < NA) p.q[r * p.q_sr + a * p.q_sa + act] = qv;
                if (act < NA && qv > best) {  // ascending ids, strictly greater: the lowest id among equal maxima
                    best = qv;
                    arg = act;
                }
            }
#pragma unroll
            for (int off = 16; off < 64; off <<= 1) {
                const float ov = __shfl_xor(best, off);
                const int oa = __shfl_xor(arg, off);
                if (ov > best || (ov == best && oa < arg)) {
                    best = ov;
                    arg = oa;
                }
            }
            if (g == 0 && ok) {
                const int id = exid >= 0 ? exid : arg;
                if (p.act_i64)
                    static_cast<int64_t*>(p.action)[r * p.a_sr + a * p.a_sa] = id;
                else
                    static_cast<float*>(p.action)[r * p.a_sr + a * p.a_sa] = (float)id;
            }
        }
    }
}

// [lo, hi) bytes covered by rows b < B, agents a < A of `width` floats at base + b*sr + a*sa
void extent(const float* base, int A, int B, int64_t sr, int64_t sa, int width, uintptr_t& lo, uintptr_t& hi) {
    const int64_t dr = (int64_t)(B - 1) * sr, da = (int64_t)(A - 1) * sa;
    const int64_t mn = (dr < 0 ? dr : 0) + (da < 0 ? da : 0), mx = (dr > 0 ? dr : 0) + (da > 0 ? da : 0);
    lo = (uintptr_t)(base + mn);
    hi = (uintptr_t)(base + mx + width);
}
}  // namespace

extern "C" int flock_vdn_act(void* stream, int A, int B, int n_obs, int n_actions, const float* w1, const float* b1,
                             const float* w2, const float* b2, const float* w_ih, const float* w_hh,
                             const float* b_ih, const float* b_hh, const float* w_q, const float* b_q,
                             const float* obs, int64_t obs_sb, int64_t obs_sa, const float* h_in, int64_t h_in_sb,
                             int64_t h_in_sa, float* h_out, int64_t h_out_sb, int64_t h_out_sa, void* action,
                             int64_t action_sb, int64_t action_sa, float* q_out, int64_t q_sb, int64_t q_sa,
                             const float* coin, const int64_t* rnd, const uint8_t* reset, float epsilon,
                             int action_int64, int row_split) {
    if (A <= 0 || B <= 0) return 0;
    if (!w1 || !b1 || !w2 || !b2 || !w_ih || !w_hh || !b_ih || !b_hh || !w_q || !b_q || !obs || !h_in || !h_out ||
        !action)
        return fail(-3, "flock_vdn_act: NULL pointer");
    if ((coin == nullptr) != (rnd == nullptr)) return fail(-3, "flock_vdn_act: coin and rnd go together");
    if (n_obs < 1 || n_obs > kFMaxIn) return fail(-2, "flock_vdn_act: n_obs must be in [1, 16]");
    if (n_actions < 1 || n_actions > kMaxAct) return fail(-2, "flock_vdn_act: n_actions must be in [1, 16]");
    const int tiles = (B + kFRows - 1) / kFRows;
    if (row_split < 0 || (int64_t)A * (row_split ? row_split : tiles) > INT32_MAX)
        return fail(-5, "flock_vdn_act: row_split must be >= 0 and A * row_split fit the grid");
    if (((uintptr_t)h_in | (uintptr_t)h_out) & 15u || ((h_in_sb | h_in_sa | h_out_sb | h_out_sa) & 3))
        return fail(-5, "flock_vdn_act: hidden rows must be 16-byte aligned");
    uintptr_t ilo, ihi, olo, ohi;
    extent(h_in, A, B, h_in_sb, h_in_sa, kH, ilo, ihi);
    extent(h_out, A, B, h_out_sb, h_out_sa, kH, olo, ohi);
    if (ilo < ohi && olo < ihi) return fail(-5, "flock_vdn_act: h_out overlaps h_in (keep two buffers and swap them)");
    int S = row_split;
    if (S == 0) {  // two rounds of three blocks on each of the 256 CUs: the last blocks to finish are short ones
        S = (1536 + A - 1) / A;
        if (S > tiles) S = tiles;
    }
    const VdnActArgs p{A, B, n_obs, n_actions, S, w1, b1, w2, b2, w_ih, w_hh, b_ih, b_hh, w_q, b_q,
                       obs, obs_sb, obs_sa, h_in, h_in_sb, h_in_sa, h_out, h_out_sb, h_out_sa,
                       action, action_sb, action_sa, q_out, q_sb, q_sa, coin, rnd, reset, epsilon, action_int64};
    hipLaunchKernelGGL(vdn_act_kernel, dim3(A * S), dim3(kBlock), 0, (hipStream_t)stream, p);
    return launched();
}
