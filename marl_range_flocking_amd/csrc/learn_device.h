// Device helpers shared by the kernels of the VDN QNet: the layer widths of the feature chain, the MFMA accumulator
// type and the sigmoid of the GRU gates (flock_learn.hip: vdn_feat_fwd/bwd and the GRU kernels; act_device.h: the GRU
// step of the fused acting kernels, whose gate math must be gru_fwd_kernel's), and the LDS strides, LDS-only workgroup
// barrier and f32 MFMA row GEMM of the training-side feature kernels. Include after `#pragma clang fp contract(off)`.
#pragma once

#include <hip/hip_runtime.h>

#include <math.h>

namespace flock_learn_device {

static __device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

constexpr int kF1 = 64, kF2 = 32, kFG = 96, kFRows = 64, kFMaxIn = 16;
constexpr int kSW1 = kFMaxIn + 2, kSY1 = kF1 + 2, kSY2 = kF2 + 2;  // LDS row strides (floats)
using f32x4_t = float __attribute__((ext_vector_type(4)));

// Workgroup barrier for LDS hand-offs only: waits for this wave's LDS operations (lgkmcnt), not for its global loads
// (__syncthreads() waits for vmcnt(0) too, which would drain the next rows' prefetch at every barrier). The global
// loads' own waits stay where their registers are first used.
static __device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// NT column tiles of 16: acc[t] += A[16 rows][K] * W[16 t .. 16 t + 16][K]^T, k in steps of 4 (one MFMA each)
template <int NT>
static __device__ __forceinline__ void mfma_rows(f32x4_t (&acc)[NT], const float* a, int sa, const float* w, int sw,
                                                 int K, int lane) {
    const int i = lane & 15, kk = lane >> 4;
    for (int k = 0; k < K; k += 4) {
        const float av = a[i * sa + k + kk];
#pragma unroll
        for (int t = 0; t < NT; ++t)
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, w[(16 * t + i) * sw + k + kk], acc[t], 0, 0, 0);
    }
}

}  // namespace flock_learn_device
