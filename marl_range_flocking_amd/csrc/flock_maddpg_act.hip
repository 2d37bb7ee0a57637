// flock_maddpg_act.hip — the acting step of the MADDPG actors for every (env row, agent) in ONE launch (gfx950).
//
// Recurrent actor (learners/maddpg_official_rnn/net.py:53-72, agent.py:53-64) per row b and agent a, agent a's weights:
//   y = fce x + b [32]      h' = GRUCell(y, h) (gru_fwd_kernel's gate math and operation order, learn_device.h)
//   y1 = relu(fc1 h' + b1) [h1]   y2 = relu(fc2 y1 + b2) [h2]
//   action = ((tanh(linear_speed y2 + b) + 1) / 2, tanh(angular_speed y2 + b) * 1.5) [+ noise[b][a][0..1]]
// Feed-forward actor (learners/maddpg_official/net.py): the same kernel with x, zero-padded to 32 wide, in place of h'
// (fc1: k -> h1), no GRU, no hidden state, and the head tanh(fc3 y2 + b) with no affine.
// The torch chain it replaces (MADDPGLearner.get_actions -> actor_forward) runs five or six batched GEMMs and the
// elementwise passes between them, with y1 [A, B, h1] and y2 [A, B, h2] through HBM; here a row moves its observation,
// its hidden state in and out, its two noise values and its two actions.
//
// Layout. A block of 4 waves owns ONE agent and walks a run of that agent's 64-row tiles; wave w takes rows [16 w,
// 16 w + 16) of each tile. Every layer is f32 MFMA (v_mfma_f32_16x16x4_f32) computed TRANSPOSED, out^T = W act^T, as
// flock_vdn_act.hip's header tells: the A operand is a weight tile from LDS, the B operand the activations from
// registers, and what lane (j, g) ends a layer with is what the next layer's B operand wants from it. So fce, both gate
// products, the GRU cell, fc1, fc2 and the two head dot products keep their activations in registers; LDS has weights.
//   Per tile, recurrent flavour: fce.weight and the two GRU matrices (26.9 KB) are staged, the GRU step runs and h' is
// stored as h was loaded: act_device.h's staging, small-input layer, gru_step and hidden-state accesses.
//   Then fc1 and fc2 run together, chunk by chunk: chunk c holds fc1.weight rows [16 c, 16 c + 16) (16 x 32, the
// 16 fc1 features that are fc2's k = 16 c .. 16 c + 15) and fc2.weight[:, 16 c .. 16 c + 15] (16 NT rows, pitch 20
// floats: the 16-B fragment reads of 8 consecutive rows fall on distinct 16-B bank groups). A wave computes its 16
// rows' 16 y1 values (8 MFMAs, bias, ReLU: 4 registers a lane) and feeds them to NT x 4 fc2 MFMAs, each weight fragment
// one 16-B LDS read for 4 MFMAs. y1 is never whole anywhere: 4 registers; y2 is the 4 NT accumulators. The chunks are
// double-buffered: one LDS-only barrier per chunk, the next chunk's global loads in flight (registers) meanwhile.
//   fc2.weight (480 KB an agent at 400 x 300) does not fit LDS, so every tile streams it from L2 as sc_act16_kernel
// does; all blocks of an agent run on one XCD (act_device.h's row_run) to keep it in that XCD's L2.
// Widths that do not fill a tile are zero-padded in LDS (weight rows and columns, biases, head rows): padded fc1
// features are relu(0) = 0 against zero fc2 columns, padded fc2 features are relu(0) = 0 against zero head weights.
// A row's result depends on that row and the weights only: not on its place in the tile, the block or the grid.
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
using namespace flock_act_device;  // kH: the GRU width = fc1's input width

constexpr int kRows = 64;              // rows per tile (16 per wave)
constexpr int kMaxIn = kFMaxIn, kMaxH1 = 512, kMaxH2 = 320;
constexpr int kKC = 16;                // fc1 features per chunk = depth of a chunk's fc2.weight slice
constexpr int kP2 = kKC + 4;           // pitch of a staged fc2.weight row (floats)
constexpr int kW1C = kKC * kH;         // a chunk's fc1.weight rows
constexpr int kSF = kMaxIn + 2;        // widest fce.weight row pitch
constexpr int kGruFloats = kH * kSF + 2 * kG * kH;  // fce.weight + weight_ih + weight_hh
constexpr int kNBias = kH + 2 * kG + 4;             // fce.bias, bias_ih, bias_hh, the two head biases (+ 2 pad)

struct MaddpgActArgs {
    int A, B, K, H1, H2, S, rec;
    const float *Wf, *bf, *Wi, *Wh, *bi, *bh, *W1, *b1, *W2, *b2, *Wa, *ba, *Wb, *bb;
    const float* obs;
    int64_t o_sr, o_sa;
    const float* hin;
    int64_t hi_sr, hi_sa;
    float* hout;
    int64_t ho_sr, ho_sa;
    float* action;
    int64_t a_sr, a_sa;
    const float* noise;
    int64_t n_sr, n_sa;
    const uint8_t* reset;
};

constexpr int lds_floats(int NT, int H1P) {
    const int chunk = 16 * NT * kP2 + kW1C;
    return H1P + 3 * 16 * NT + kNBias + (2 * chunk > kGruFloats ? 2 * chunk : kGruFloats);
}
static_assert(lds_floats(kMaxH2 / 16, kMaxH1) * sizeof(float) <= 64 * 1024, "two blocks per CU at the widest network");

// NT: 16-feature tiles of fc2's output (h2 <= 16 NT). Two waves per SIMD (at most 256 registers).
template <int NT>
__global__ __launch_bounds__(kBlock, 2) void maddpg_act_kernel(MaddpgActArgs p) {
    constexpr int NC = 16 * NT, CF = NC * kP2 + kW1C;
    constexpr int NPF = (NC * (kKC / 4) + kBlock - 1) / kBlock;  // float4 of fc2.weight per thread per chunk
    extern __shared__ float4 smem4[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int K = p.K, H1 = p.H1, H2 = p.H2, H1P = (H1 + 15) & ~15, NCH = H1P >> 4;
    const bool rec = p.rec != 0;
    // LDS: fc1.bias [H1P], fc2.bias / head row 0 / head row 1 [NC each], the small biases, then the region that holds
    // the GRU-stage weights or the two chunk buffers
    float* sB1 = reinterpret_cast<float*>(smem4);
    float *sB2 = sB1 + H1P, *sHA = sB2 + NC, *sHB = sHA + NC, *sBs = sHB + NC, *U = sBs + kNBias;
    const float *bsf = sBs, *bsi = sBs + kH, *bsh = bsi + kG, *bsa = bsh + kG;

    const RowRun run = row_run(p.A, p.S, p.B, kRows);
    const int64_t a = run.a, r_begin = run.r_begin, r_end = run.r_end;
    if (r_begin >= r_end) return;

    for (int e = tid; e < H1P; e += kBlock) sB1[e] = e < H1 ? p.b1[a * H1 + e] : 0.0f;
    for (int c = tid; c < NC; c += kBlock) {
        const bool v = c < H2;
        sB2[c] = v ? p.b2[a * H2 + c] : 0.0f;
        sHA[c] = v ? (rec ? p.Wa[a * H2 + c] : p.Wa[2 * a * H2 + c]) : 0.0f;
        sHB[c] = v ? (rec ? p.Wb[a * H2 + c] : p.Wa[(2 * a + 1) * H2 + c]) : 0.0f;
    }
    if (rec) {
        if (tid < kH) sBs[tid] = p.bf[a * kH + tid];
        if (tid < kG) {
            sBs[kH + tid] = p.bi[a * kG + tid];
            sBs[kH + kG + tid] = p.bh[a * kG + tid];
        }
    }
    if (tid < 2) sBs[kH + 2 * kG + tid] = rec ? (tid == 0 ? p.ba[a] : p.bb[a]) : p.ba[2 * a + tid];
    // (made visible by the tile loop's first barrier, before anything reads it)

    const int j = lane & 15, g = lane >> 4;
    const int m = (4 * g) ^ swz(j);  // k = c + 4 g of a swizzled row i = j sits at column c ^ m
    const int in1 = rec ? kH : K;    // fc1's input width
    const float* W1a = p.W1 + a * H1 * in1;
    const float* W2a = p.W2 + a * H2 * H1;
    const int K1 = (K + 3) & ~3, sx = K1 + 2;  // fce's row pitch
    float *wf = U, *wi = U + kH * kSF, *wh = wi + kG * kH;

    // one chunk's weights on their way from global memory to LDS
    float4 pw[NPF];
    float p1[2];
    const int o1 = tid >> 4, kk = tid & 15;
    auto fetch = [&](int c) {
        const int k0 = kKC * c;
#pragma unroll
        for (int i = 0; i < NPF; ++i) {
            const int e = tid + kBlock * i, o = e >> 2, q = 4 * (e & 3);
            pw[i] = (o < H2 && k0 + q < H1) ? *reinterpret_cast<const float4*>(W2a + (int64_t)o * H1 + k0 + q)
                                            : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
        const int f = k0 + o1;
        p1[0] = (f < H1 && kk < in1) ? W1a[(int64_t)f * in1 + kk] : 0.0f;
        p1[1] = (f < H1 && kk + 16 < in1) ? W1a[(int64_t)f * in1 + kk + 16] : 0.0f;
    };
    auto stage = [&](float* buf) {
#pragma unroll
        for (int i = 0; i < NPF; ++i) {
            const int e = tid + kBlock * i, o = e >> 2, q = 4 * (e & 3);
            if (o < NC) *reinterpret_cast<float4*>(buf + o * kP2 + q) = pw[i];
        }
        float* w1 = buf + NC * kP2 + o1 * kH;
        w1[kk ^ swz(o1)] = p1[0];
        w1[(kk + 16) ^ swz(o1)] = p1[1];
    };

    for (int64_t r0 = r_begin; r0 < r_end; r0 += kRows) {
        const int64_t r = r0 + 16 * wv + j;  // this lane's row
        const bool ok = r < r_end;
        fetch(0);
        float nz = 0.0f;  // lane groups 0 and 1: the row's noise for action component g
        if (p.noise && ok && g < 2) nz = p.noise[r * p.n_sr + a * p.n_sa + g];
        float hv[2][4];  // fc1's input: element 16 T + 4 g + v of row j
        if (rec) {
            float x[kMaxIn / 4], h[2][4];
#pragma unroll
            for (int s4 = 0; s4 < kMaxIn / 4; ++s4)
                x[s4] = (ok && 4 * s4 + g < K) ? p.obs[r * p.o_sr + a * p.o_sa + 4 * s4 + g] : 0.0f;
            float4 hr[2] = {make_float4(0.0f, 0.0f, 0.0f, 0.0f), make_float4(0.0f, 0.0f, 0.0f, 0.0f)};
            if (ok && !(p.reset && p.reset[r])) load_h(hr, p.hin + r * p.hi_sr + a * p.hi_sa + 4 * g);  // else h = 0
            unpack_h(h, hr, false);
            lds_barrier();  // the previous tile's last chunk has been read
            stage_small_in(wf, p.Wf, a, kH, K, tid);
            stage_gates(wi, wh, p.Wi, p.Wh, a, tid);
            lds_barrier();
            float y[2][4];
            {  // fce: 2 feature tiles, k = 4 s + g
                f32x4_t acc[2] = {};
                small_in_layer<2>(acc, wf + j * sx + g, K1, x);
#pragma unroll
                for (int T = 0; T < 2; ++T)
#pragma unroll
                    for (int v = 0; v < 4; ++v) y[T][v] = acc[T][v] + bsf[16 * T + 4 * g + v];
            }
            gru_step(hv, y, h, wi + j * kH, wh + j * kH, bsi, bsh, m, g);
            if (ok) store_h(p.hout + r * p.ho_sr + a * p.ho_sa + 4 * g, hv);  // h' as h was loaded
        } else {
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                hv[0][v] = (ok && 4 * g + v < K) ? p.obs[r * p.o_sr + a * p.o_sa + 4 * g + v] : 0.0f;
                hv[1][v] = 0.0f;  // K <= 16
            }
        }
        lds_barrier();  // the GRU-stage weights (or the previous tile's last chunk) have been read
        stage(U);
        if (NCH > 1) fetch(1);

        f32x4_t acc[NT] = {};
        for (int c = 0; c < NCH; ++c) {
            lds_barrier();  // chunk c is staged; the other buffer's chunk c - 1 has been read
            if (c + 1 < NCH) {
                stage(U + ((c + 1) & 1) * CF);
                if (c + 2 < NCH) fetch(c + 2);
            }
            const float* buf = U + (c & 1) * CF;
            const float* w2l = buf + j * kP2 + 4 * g;  // fc2.weight[16 T + j][16 c + 4 g .. + 3]
            auto frag = [&](int T) { return *reinterpret_cast<const float4*>(w2l + 16 * T * kP2); };
            // the weight fragments run two tiles ahead of their MFMAs (the LDS latency of one read is 4 MFMAs long)
            float4 wq[3];
            wq[0] = frag(0);
            if (NT > 1) wq[1] = frag(1);
            float y1[4];
            {  // fc1 features 16 c + 4 g + v of row j
                const float* w1l = buf + NC * kP2 + j * kH;
                float w1v[2][4];
#pragma unroll
                for (int Tp = 0; Tp < 2; ++Tp)
#pragma unroll
                    for (int v = 0; v < 4; ++v) w1v[Tp][v] = w1l[(16 * Tp + v) ^ m];
                f32x4_t a1 = {};
#pragma unroll
                for (int Tp = 0; Tp < 2; ++Tp)
#pragma unroll
                    for (int v = 0; v < 4; ++v)
                        a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w1v[Tp][v], hv[Tp][v], a1, 0, 0, 0);
                const float4 bb = *reinterpret_cast<const float4*>(sB1 + kKC * c + 4 * g);
                y1[0] = fmaxf(a1[0] + bb.x, 0.0f), y1[1] = fmaxf(a1[1] + bb.y, 0.0f);
                y1[2] = fmaxf(a1[2] + bb.z, 0.0f), y1[3] = fmaxf(a1[3] + bb.w, 0.0f);
            }
#pragma unroll
            for (int T = 0; T < NT; ++T) {
                if (T + 2 < NT) wq[(T + 2) % 3] = frag(T + 2);
                const float4 wc = wq[T % 3];
                acc[T] = __builtin_amdgcn_mfma_f32_16x16x4f32(wc.x, y1[0], acc[T], 0, 0, 0);
                acc[T] = __builtin_amdgcn_mfma_f32_16x16x4f32(wc.y, y1[1], acc[T], 0, 0, 0);
                acc[T] = __builtin_amdgcn_mfma_f32_16x16x4f32(wc.z, y1[2], acc[T], 0, 0, 0);
                acc[T] = __builtin_amdgcn_mfma_f32_16x16x4f32(wc.w, y1[3], acc[T], 0, 0, 0);
            }
        }

        // heads: this lane's 4 NT fc2 features against the two head rows, then the row's four lanes
        float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
        for (int T = 0; T < NT; ++T) {
            const float4 b2 = *reinterpret_cast<const float4*>(sB2 + 16 * T + 4 * g);
            const float4 ha = *reinterpret_cast<const float4*>(sHA + 16 * T + 4 * g);
            const float4 hb = *reinterpret_cast<const float4*>(sHB + 16 * T + 4 * g);
            const float e0 = fmaxf(acc[T][0] + b2.x, 0.0f), e1 = fmaxf(acc[T][1] + b2.y, 0.0f),
                        e2 = fmaxf(acc[T][2] + b2.z, 0.0f), e3 = fmaxf(acc[T][3] + b2.w, 0.0f);
            s0 += e0 * ha.x, s0 += e1 * ha.y, s0 += e2 * ha.z, s0 += e3 * ha.w;
            s1 += e0 * hb.x, s1 += e1 * hb.y, s1 += e2 * hb.z, s1 += e3 * hb.w;
        }
        s0 += __shfl_xor(s0, 16), s0 += __shfl_xor(s0, 32);
        s1 += __shfl_xor(s1, 16), s1 += __shfl_xor(s1, 32);
        if (ok && g < 2) {  // lane group 0 writes the first action component, group 1 the second
            float u = tanhf((g ? s1 : s0) + bsa[g]);
            if (rec) u = g ? u * 1.5f : (u + 1.0f) / 2.0f;
            if (p.noise) u = u + nz;
            p.action[r * p.a_sr + a * p.a_sa + g] = u;
        }
    }
}

template <int NT>
int launch(hipStream_t st, const MaddpgActArgs& p) {
    const size_t lds = sizeof(float) * (size_t)lds_floats(NT, (p.H1 + 15) & ~15);
    hipLaunchKernelGGL(maddpg_act_kernel<NT>, dim3(p.A * p.S), dim3(kBlock), lds, st, p);
    return launched();
}
}  // namespace

extern "C" int flock_maddpg_act(void* stream, int A, int B, int k, int h1, int h2, int recurrent, const float* fce_w,
                                const float* fce_b, const float* w_ih, const float* w_hh, const float* b_ih,
                                const float* b_hh, const float* fc1_w, const float* fc1_b, const float* fc2_w,
                                const float* fc2_b, const float* head_w, const float* head_b, const float* head2_w,
                                const float* head2_b, const float* obs, int64_t obs_sb, int64_t obs_sa,
                                const float* h_in, int64_t h_in_sb, int64_t h_in_sa, float* h_out, int64_t h_out_sb,
                                int64_t h_out_sa, float* action, int64_t action_sb, int64_t action_sa,
                                const float* noise, int64_t noise_sb, int64_t noise_sa, const uint8_t* reset,
                                int row_split) {
    if (A <= 0 || B <= 0) return 0;
    if (!fc1_w || !fc1_b || !fc2_w || !fc2_b || !head_w || !head_b || !obs || !action)
        return fail(-3, "flock_maddpg_act: NULL pointer");
    if (recurrent && (!fce_w || !fce_b || !w_ih || !w_hh || !b_ih || !b_hh || !head2_w || !head2_b || !h_in || !h_out))
        return fail(-3, "flock_maddpg_act: NULL pointer (the recurrent actor needs fce, the GRU, both heads, h_in, h_out)");
    if (k < 1 || k > kMaxIn) return fail(-2, "flock_maddpg_act: k must be in [1, 16]");
    if (h1 < 8 || h1 > kMaxH1 || (h1 & 7)) return fail(-2, "flock_maddpg_act: h1 must be a multiple of 8 in [8, 512]");
    if (h2 < 1 || h2 > kMaxH2) return fail(-2, "flock_maddpg_act: h2 must be in [1, 320]");
    // automatic split: about eight work items for each of the 512 resident blocks, so the last to finish are short
    int S;
    if (int rc = row_split_of("flock_maddpg_act", A, B, kRows, row_split, 4096, S)) return rc;
    if ((uintptr_t)fc2_w & 15u) return fail(-5, "flock_maddpg_act: fc2.weight must be 16-byte aligned");
    if (recurrent)
        if (int rc = check_hidden_pair("flock_maddpg_act", A, B, kH, h_in, h_in_sb, h_in_sa, h_out, h_out_sb, h_out_sa))
            return rc;
    const MaddpgActArgs p{A, B, k, h1, h2, S, recurrent ? 1 : 0, fce_w, fce_b, w_ih, w_hh, b_ih, b_hh, fc1_w, fc1_b,
                          fc2_w, fc2_b, head_w, head_b, head2_w, head2_b, obs, obs_sb, obs_sa, h_in, h_in_sb, h_in_sa,
                          h_out, h_out_sb, h_out_sa, action, action_sb, action_sa, noise, noise_sb, noise_sa, reset};
    hipStream_t st = (hipStream_t)stream;
    const int nt = (h2 + 15) / 16;
    if (nt <= 2) return launch<2>(st, p);
    if (nt <= 4) return launch<4>(st, p);
    if (nt <= 8) return launch<8>(st, p);
    if (nt <= 12) return launch<12>(st, p);
    if (nt <= 16) return launch<16>(st, p);
    if (nt <= 19) return launch<19>(st, p);
    return launch<20>(st, p);
}
