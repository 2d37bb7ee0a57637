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
// The same holds for the hidden state, both gate products and h' (act_device.h's load_h, gru_step and store_h: the GRU
// cell runs in registers) and for the q head, whose 16 outputs per row lie 4 to a lane: argmax is a scan of those 4 and
// two xor steps (lanes 16 and 32 apart) carrying (value, index).
// x is loaded by the lane that feeds it to layer 1 (k = 4 s + g). The next 16 rows' x, h, reset flag, coin and random
// id are in flight while the current ones compute. A row's result depends on nothing but that row and the weights:
// not on its place in the tile, the block or the grid.
// LDS (floats): W1 64 x (K1 + 2), W2 32 x 64, Wih 96 x 32, Whh 96 x 32, Wq 16 x 32 (rows >= n_actions zero), biases
// 304: 10160 floats = 40.6 KB. W2 / Wih / Whh / Wq rows are unpadded and XOR-swizzled. The swizzle, the staging of W1
// and the gate matrices, layer 1's MFMA loop, the GRU step, the hidden-state accesses and the split of an agent's rows
// over blocks (work item -> block in XCD order) are act_device.h's, shared with flock_maddpg_act.hip.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "act_host.h"
#include "flock_learn.h"

#pragma clang fp contract(off)

#include "act_device.h"

namespace {
using flock_learn_internal::fail;
using flock_learn_internal::launched;
using namespace flock_act_host;
using namespace flock_act_device;

constexpr int kMaxAct = 16;  // one q tile
constexpr int kNBias = kF1 + kF2 + 2 * kG + kMaxAct;
// LDS offsets (floats)
constexpr int oW1 = 0, oW2 = oW1 + kF1 * kSW1, oWi = oW2 + kF2 * kF1, oWh = oWi + kG * kH, oWq = oWh + kG * kH,
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

// three waves per SIMD (at most 168 registers): with 40.6 KB of LDS, three blocks per CU
__global__ __launch_bounds__(kBlock, 3) void vdn_act_kernel(VdnActArgs p) {
    __shared__ __attribute__((aligned(16))) float sm[kLdsFloats];
    float *w1 = sm + oW1, *w2 = sm + oW2, *wi = sm + oWi, *wh = sm + oWh, *wq = sm + oWq, *bs = sm + oBs;
    const float *bs1 = bs, *bs2 = bs + kF1, *bsi = bs2 + kF2, *bsh = bsi + kG, *bsq = bsh + kG;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const RowRun run = row_run(p.A, p.S, p.B, kFRows);
    const int64_t a = run.a, r_begin = run.r_begin, r_end = run.r_end;
    if (r_begin >= r_end) return;

    const int NI = p.NI, NA = p.NA, K1 = (NI + 3) & ~3, sx = K1 + 2;  // sx: w1's row pitch
    stage_small_in(w1, p.W1, a, kF1, NI, tid);
    for (int e = tid; e < kF2 * kF1; e += kBlock) {
        const int o = e / kF1, k = e % kF1;
        w2[o * kF1 + (k ^ swz(o & 15))] = p.W2[a * kF2 * kF1 + e];
    }
    stage_gates(wi, wh, p.Wi, p.Wh, a, tid);
    for (int e = tid; e < kMaxAct * kH; e += kBlock) {
        const int o = e / kH, k = e % kH;
        wq[o * kH + (k ^ swz(o))] = e < NA * kH ? p.Wq[a * NA * kH + e] : 0.0f;
    }
    if (tid < kF1) bs[tid] = p.b1[a * kF1 + tid];
    if (tid < kF2) bs[kF1 + tid] = p.b2[a * kF2 + tid];
    if (tid < kG) {
        bs[kF1 + kF2 + tid] = p.bi[a * kG + tid];
        bs[kF1 + kF2 + kG + tid] = p.bh[a * kG + tid];
    }
    if (tid < kMaxAct) bs[kF1 + kF2 + 2 * kG + tid] = tid < NA ? p.bq[a * NA + tid] : 0.0f;
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
            load_h(hr, p.hin + r * p.hi_sr + a * p.hi_sa + 4 * g);
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
        unpack_h(h, hr, rs != 0);
        const int exid = (explore && cn <= p.eps) ? (int)rn : -1;  // lanes 0..15: the row's exploration id
        if (r0 + kFRows < r_end) load(r + kFRows);                 // in flight while these rows compute

        float y1[4][4], y2[2][4];
        {  // layer 1: 4 feature tiles, k = 4 s + g
            f32x4_t acc[4] = {};
            small_in_layer<4>(acc, w1l, K1, x);
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
        gru_step(ho, y2, h, wil, whl, bsi, bsh, m, g);
        if (ok) store_h(p.hout + r * p.ho_sr + a * p.ho_sa + 4 * g, ho);  // h' as h was loaded
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
    // automatic split: two rounds of three blocks on each of the 256 CUs, so the last blocks to finish are short ones
    int S;
    if (int rc = row_split_of("flock_vdn_act", A, B, kFRows, row_split, 1536, S)) return rc;
    if (int rc = check_hidden_pair("flock_vdn_act", A, B, kH, h_in, h_in_sb, h_in_sa, h_out, h_out_sb, h_out_sa))
        return rc;
    const VdnActArgs p{A, B, n_obs, n_actions, S, w1, b1, w2, b2, w_ih, w_hh, b_ih, b_hh, w_q, b_q,
                       obs, obs_sb, obs_sa, h_in, h_in_sb, h_in_sa, h_out, h_out_sb, h_out_sa,
                       action, action_sb, action_sa, q_out, q_sb, q_sa, coin, rnd, reset, epsilon, action_int64};
    hipLaunchKernelGGL(vdn_act_kernel, dim3(A * S), dim3(kBlock), 0, (hipStream_t)stream, p);
    return launched();
}
