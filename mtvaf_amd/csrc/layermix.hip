// Layer mix (mtvaf_amd/modules/layer_mix.py, engine.EncoderMixFunction; new functionality, the reference's heads read the last
// layer only): y = gamma * sum_j softmax(scalars)_j * h_{k_j} over K <= 32 chosen hidden states, and what its backward needs.
// DESIGN.md section 4.26.
//
//   mtvaf_layer_mix_fwd     K state pointers (a by-value table in the kernel arguments), scalars [K] and gamma [1] on the device
//                           -> y [rows,H].  s = softmax(scalars) is recomputed by every block with the arithmetic of lm_softmax.
//   mtvaf_layer_mix_dots    t_j = sum_{r,c} dy * h_{k_j} in double: stage 1 leaves one partial per block and state, the finalize
//                           block adds them in a fixed order and writes d scalars [K], d gamma [1] and the coefficients
//                           c_j = gamma * s_j [K] the injection reads.
//   mtvaf_layer_mix_inject  dh = fmaf(c_j, dy, dh), or dh = c_j * dy where no dh exists yet: the gradient of state k_j is never
//                           materialised, the encoder backward adds it into its running dh at the boundary of layer k_j.
//
// No atomics, no host synchronisation, a launch geometry that depends on (rows, H, K) alone: the same inputs give the same bits.
#include "common.h"

namespace mtvaf {

constexpr int LM_THREADS = 256;
constexpr int LM_MAX_BLOCKS = 2048;                        // element-wise kernels: 8 blocks per CU
constexpr int LM_DOT_BLOCKS = MTVAF_LAYER_MIX_DOT_BLOCKS;  // stage-1 blocks of the dots (the workspace holds K x this many doubles)
constexpr int LM_GROUP = 8;                                // states per sweep over dy in the dots

struct LmTable {
  const float* p[MTVAF_LAYER_MIX_MAX_K];
};

// The arithmetic of the mix, stated once.  Nothing here may be contracted or re-associated: the bits follow from this text.
//   s_j = expf(a_j - max a) / (e_0 + e_1 + ... + e_{K-1}), the sum taken in that order; one correctly rounded division each
//   y   = gamma * fmaf(s_{K-1}, h_{K-1}, ... fmaf(s_1, h_1, fmaf(s_0, h_0, 0)))
__device__ __forceinline__ float lm_fma(float a, float b, float c) { return __fmaf_rn(a, b, c); }
__device__ __forceinline__ float lm_mul(float a, float b) {
#pragma clang fp contract(off)
  return __fmul_rn(a, b);
}

// softmax(scalars) into s[0..K) (LDS), by the whole block (at least one wave); ends with a barrier.
__device__ __forceinline__ void lm_softmax(const float* __restrict__ scalars, int K, float* s, float* sum) {
#pragma clang fp contract(off)
  const int t = threadIdx.x;
  if (t < 64) {
    const float a = t < K ? scalars[t] : -INFINITY;
    const float mx = wave_max(a);  // (a maximum does not depend on the order it is taken in)
    if (t < K) s[t] = expf(__fsub_rn(a, mx));
  }
  __syncthreads();
  if (t == 0) {
    float acc = 0.f;
    for (int j = 0; j < K; ++j) acc = __fadd_rn(acc, s[j]);
    *sum = acc;
  }
  __syncthreads();
  if (t < K) s[t] = __fdiv_rn(s[t], *sum);
  __syncthreads();
}

__global__ __launch_bounds__(LM_THREADS) void layer_mix_fwd_kernel(LmTable tab, const float* __restrict__ scalars,
                                                                   const float* __restrict__ gamma, float* __restrict__ y, long n4,
                                                                   int K) {
  __shared__ float s[MTVAF_LAYER_MIX_MAX_K];
  __shared__ float sum;
  lm_softmax(scalars, K, s, &sum);
  const float g = gamma[0];
  for (long i = (long)blockIdx.x * LM_THREADS + threadIdx.x; i < n4; i += (long)gridDim.x * LM_THREADS) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int j = 0; j < K; ++j) {
      const f32x4 h = reinterpret_cast<const f32x4*>(tab.p[j])[i];
      const float sj = s[j];
      acc = f32x4{lm_fma(sj, h.x, acc.x), lm_fma(sj, h.y, acc.y), lm_fma(sj, h.z, acc.z), lm_fma(sj, h.w, acc.w)};
    }
    reinterpret_cast<f32x4*>(y)[i] = f32x4{lm_mul(g, acc.x), lm_mul(g, acc.y), lm_mul(g, acc.z), lm_mul(g, acc.w)};
  }
}

__device__ __forceinline__ double lm_wave_sum(double v) {  // a fixed tree: the same lanes meet in the same order every time
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Stage 1: partial[j * gridDim.x + block] = this block's share of t_j.  Every thread walks its elements in ascending order, the
// wave and the block add in a fixed tree.  LM_GROUP states share one sweep over dy, their accumulators stay in registers.
__global__ __launch_bounds__(LM_THREADS) void layer_mix_dots_kernel(LmTable tab, const float* __restrict__ dy,
                                                                    double* __restrict__ partial, long n4, int K) {
  __shared__ double red[LM_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int j0 = 0; j0 < K; j0 += LM_GROUP) {
    double acc[LM_GROUP];
    const float* hp[LM_GROUP];
#pragma unroll
    for (int u = 0; u < LM_GROUP; ++u) {
      acc[u] = 0.0;
      hp[u] = tab.p[j0 + u < K ? j0 + u : j0];  // (a state past K: read again what is in cache, the sum is dropped below)
    }
    for (long i = (long)blockIdx.x * LM_THREADS + threadIdx.x; i < n4; i += (long)gridDim.x * LM_THREADS) {
      const f32x4 d = reinterpret_cast<const f32x4*>(dy)[i];
#pragma unroll
      for (int u = 0; u < LM_GROUP; ++u) {
        const f32x4 h = reinterpret_cast<const f32x4*>(hp[u])[i];
        acc[u] = fma((double)d.x, (double)h.x, acc[u]);
        acc[u] = fma((double)d.y, (double)h.y, acc[u]);
        acc[u] = fma((double)d.z, (double)h.z, acc[u]);
        acc[u] = fma((double)d.w, (double)h.w, acc[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < LM_GROUP; ++u) {
      const double w = lm_wave_sum(acc[u]);
      __syncthreads();  // (the slots of the state before this one have been read)
      if (lane == 0) red[wave] = w;
      __syncthreads();
      if (threadIdx.x == 0 && j0 + u < K) {
        double t = red[0];
        for (int k = 1; k < LM_THREADS / 64; ++k) t += red[k];
        partial[(long)(j0 + u) * gridDim.x + blockIdx.x] = t;
      }
    }
  }
}

// Stage 2, one block: t_j = the partials of state j, lane l adding those of blocks l, l + 64, ... in ascending order, then the fixed
// tree; then  S = sum_j s_j t_j (ascending j, double),  d gamma = S,  d scalars_j = gamma s_j (t_j - S),  c_j = gamma * s_j (fp32,
// the coefficient the injection multiplies by).
__global__ __launch_bounds__(LM_THREADS) void layer_mix_finalize_kernel(const double* __restrict__ partial, int nblocks,
                                                                        const float* __restrict__ scalars,
                                                                        const float* __restrict__ gamma, float* __restrict__ dscalars,
                                                                        float* __restrict__ dgamma, float* __restrict__ coef, int K) {
  __shared__ float s[MTVAF_LAYER_MIX_MAX_K];
  __shared__ float sum;
  __shared__ double t[MTVAF_LAYER_MIX_MAX_K];
  __shared__ double S;
  lm_softmax(scalars, K, s, &sum);
  const int lane = threadIdx.x & 63;
  for (int j = threadIdx.x >> 6; j < K; j += LM_THREADS / 64) {
    double a = 0.0;
    for (int b = lane; b < nblocks; b += 64) a += partial[(long)j * nblocks + b];
    a = lm_wave_sum(a);
    if (lane == 0) t[j] = a;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0;
    for (int j = 0; j < K; ++j) a = fma((double)s[j], t[j], a);
    S = a;
    dgamma[0] = (float)a;
  }
  __syncthreads();
  if (threadIdx.x < K) {
    const float g = gamma[0];
    const int j = threadIdx.x;
    dscalars[j] = (float)((double)g * (double)s[j] * (t[j] - S));
    coef[j] = lm_mul(g, s[j]);
  }
}

template <bool ACC>
__global__ __launch_bounds__(LM_THREADS) void layer_mix_inject_kernel(const float* __restrict__ coef, int j,
                                                                      const float* __restrict__ dy, float* __restrict__ dh,
                                                                      long n4) {
  const float c = coef[j];
  for (long i = (long)blockIdx.x * LM_THREADS + threadIdx.x; i < n4; i += (long)gridDim.x * LM_THREADS) {
    const f32x4 d = reinterpret_cast<const f32x4*>(dy)[i];
    f32x4 o;
    if (ACC) {
      const f32x4 a = reinterpret_cast<const f32x4*>(dh)[i];
      o = f32x4{lm_fma(c, d.x, a.x), lm_fma(c, d.y, a.y), lm_fma(c, d.z, a.z), lm_fma(c, d.w, a.w)};
    } else {
      o = f32x4{lm_mul(c, d.x), lm_mul(c, d.y), lm_mul(c, d.z), lm_mul(c, d.w)};
    }
    reinterpret_cast<f32x4*>(dh)[i] = o;
  }
}

static inline unsigned lm_grid(long n4, int max_blocks) {
  const long blocks = (n4 + LM_THREADS - 1) / LM_THREADS;
  return (unsigned)(blocks < max_blocks ? blocks : max_blocks);
}

// The table of the K states, checked: every pointer non-NULL and 16-byte aligned.
static inline int lm_table(const float* const* states, int K, LmTable* tab) {
  if (K < 1 || K > MTVAF_LAYER_MIX_MAX_K || !states) return MTVAF_ERR_ARG;
  uintptr_t all = 0;
  for (int j = 0; j < MTVAF_LAYER_MIX_MAX_K; ++j) {
    tab->p[j] = j < K ? states[j] : nullptr;
    if (j < K && !states[j]) return MTVAF_ERR_ARG;
    if (j < K) all |= (uintptr_t)states[j];
  }
  return (all & 15) ? MTVAF_ERR_ALIGN : MTVAF_OK;
}

}  // namespace mtvaf

using namespace mtvaf;

extern "C" {

int mtvaf_layer_mix_fwd(const float* const* states, int K, const float* scalars, const float* gamma, float* y, long rows, int H,
                        hipStream_t stream) {
  LmTable tab;
  const int rc = lm_table(states, K, &tab);
  if (rc == MTVAF_ERR_ARG || !scalars || !gamma || !y || (H & 3)) return MTVAF_ERR_ARG;
  if (rows < 1 || H < 4) return MTVAF_ERR_SHAPE;
  if (rc != MTVAF_OK || ((uintptr_t)y & 15) || (((uintptr_t)scalars | (uintptr_t)gamma) & 3)) return MTVAF_ERR_ALIGN;
  const long n4 = rows * (H >> 2);
  hipLaunchKernelGGL(layer_mix_fwd_kernel, dim3(lm_grid(n4, LM_MAX_BLOCKS)), dim3(LM_THREADS), 0, stream, tab, scalars, gamma, y, n4,
                     K);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

int mtvaf_layer_mix_dots(const float* const* states, int K, const float* dy, const float* scalars, const float* gamma, long rows,
                         int H, void* workspace, long workspace_bytes, float* dscalars, float* dgamma, float* coef,
                         hipStream_t stream) {
  LmTable tab;
  const int rc = lm_table(states, K, &tab);
  if (rc == MTVAF_ERR_ARG || !dy || !scalars || !gamma || !workspace || !dscalars || !dgamma || !coef || (H & 3)) return MTVAF_ERR_ARG;
  if (rows < 1 || H < 4) return MTVAF_ERR_SHAPE;
  if (workspace_bytes < MTVAF_LAYER_MIX_WORKSPACE_BYTES) return MTVAF_ERR_WORKSPACE;
  if (rc != MTVAF_OK || ((uintptr_t)dy & 15) || ((uintptr_t)workspace & 7) ||
      (((uintptr_t)scalars | (uintptr_t)gamma | (uintptr_t)dscalars | (uintptr_t)dgamma | (uintptr_t)coef) & 3))
    return MTVAF_ERR_ALIGN;
  const long n4 = rows * (H >> 2);
  const unsigned nb = lm_grid(n4, LM_DOT_BLOCKS);
  double* partial = static_cast<double*>(workspace);
  hipLaunchKernelGGL(layer_mix_dots_kernel, dim3(nb), dim3(LM_THREADS), 0, stream, tab, dy, partial, n4, K);
  MTVAF_LAUNCH_CHECK();
  hipLaunchKernelGGL(layer_mix_finalize_kernel, dim3(1), dim3(LM_THREADS), 0, stream, partial, (int)nb, scalars, gamma, dscalars,
                     dgamma, coef, K);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

int mtvaf_layer_mix_inject(const float* coef, int j, int K, const float* dy, float* dh, long rows, int H, int accumulate,
                           hipStream_t stream) {
  if (K < 1 || K > MTVAF_LAYER_MIX_MAX_K || j < 0 || j >= K || !coef || !dy || !dh || (H & 3)) return MTVAF_ERR_ARG;
  if (rows < 1 || H < 4) return MTVAF_ERR_SHAPE;
  if ((((uintptr_t)dy | (uintptr_t)dh) & 15) || ((uintptr_t)coef & 3)) return MTVAF_ERR_ALIGN;
  const long n4 = rows * (H >> 2);
  const dim3 grid(lm_grid(n4, LM_MAX_BLOCKS)), block(LM_THREADS);
  if (accumulate)
    hipLaunchKernelGGL(layer_mix_inject_kernel<true>, grid, block, 0, stream, coef, j, dy, dh, n4);
  else
    hipLaunchKernelGGL(layer_mix_inject_kernel<false>, grid, block, 0, stream, coef, j, dy, dh, n4);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

}  // extern "C"
