// Helpers shared by the chain kernels of the CRF head above crf.hip's 16-tag DPP kernels: crf_wide.hip, crf_lattice.hip,
// crf_risk.hip, crf_path.hip (one wavefront per sentence, tag j on lane j, the step's product a lane broadcast through LDS) and
// crf_entities.hip, crf_chunks.hip, crf_nbest.hip, crf_sample.hip (rows read across lanes, trans staged in the LDS).  Each helper
// backs a documented contract of those files -- exact zeros, results bit-identical in every lane, a length of at least 1 -- so it
// is written once, here.  Everything is inlined into the including file and compiled under THAT file's flags: crf_lattice.hip
// is built with -ffp-contract=off, the others with the library's -ffp-contract=fast (param_reduce below).
#pragma once
#include "common.h"

namespace mtvaf {

constexpr int CRF_CHAIN_CMAX = 64;                   // tags: one per lane
constexpr int CRF_CHAIN_SMAX = 512;                  // columns of a sentence
constexpr int CRF_CHAIN_LD = CRF_CHAIN_CMAX + 1;     // row stride of trans in the LDS: rows and columns both spread over the banks
constexpr float NEG = -1.0e30f;                      // the neutral element of max-plus in lanes >= C
typedef float f4 __attribute__((ext_vector_type(4)));

// one wave: LDS operations execute in program order, the fences keep the compiler from moving them across
__device__ __forceinline__ void lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// lane i of x for the whole wave (i wave-uniform)
__device__ __forceinline__ float lane_val(float x, int i) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), i));
}
__device__ __forceinline__ int lane_val(int x, int i) { return __builtin_amdgcn_readlane(x, i); }

// len_b: the leading ones of the mask row (at least 1: mask[:,0] == 1 is the caller's contract).  crf_nbest.hip and
// crf_sample.hip find the same length by ballot and keep that loop, with the same max(len, 1), in their kernels: behind a call
// it compiles to other instructions
__device__ __forceinline__ int prefix_len(const uint8_t* __restrict__ mrow, int S, int lane) {
  int len = S;
  for (int t = lane; t < S; t += 64)
    if (!mrow[t]) len = min(len, t);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) len = min(len, __shfl_xor(len, o, 64));
  return max(len, 1);
}

// max over the C x C transitions, the same value in every lane
__device__ __forceinline__ float trans_max(const float* __restrict__ trans, int C, int lane) {
  float tm = NEG;
  if (lane < C)
    for (int i = 0; i < C; ++i) tm = fmaxf(tm, trans[i * C + lane]);
  return wave_max(tm);
}

// trans [C,C] into its LDS image [CRF_CHAIN_CMAX][CRF_CHAIN_LD], by the `threads` threads of the block (the caller's barrier
// follows)
__device__ __forceinline__ void stage_trans(float* s_trans, const float* __restrict__ trans, int C, int tid, int threads) {
  for (int i = tid; i < C * C; i += threads) s_trans[(i / C) * CRF_CHAIN_LD + i % C] = trans[i];
}

// sum_i v[i] w[i] and sum_i v[i] over the CT values of a broadcast row; the same additions in every lane
template <int CT>
__device__ __forceinline__ void dot_sum(const float* row, const float (&w)[CT], float& dot, float& sum) {
  const f4* r4 = reinterpret_cast<const f4*>(row);
  float d0 = 0.f, d1 = 0.f, d2 = 0.f, d3 = 0.f, s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
  for (int q = 0; q < CT / 4; ++q) {
    const f4 x = r4[q];
    d0 = __builtin_fmaf(x.x, w[4 * q], d0);
    d1 = __builtin_fmaf(x.y, w[4 * q + 1], d1);
    d2 = __builtin_fmaf(x.z, w[4 * q + 2], d2);
    d3 = __builtin_fmaf(x.w, w[4 * q + 3], d3);
    s0 += x.x;
    s1 += x.y;
    s2 += x.z;
    s3 += x.w;
  }
  dot = (d0 + d1) + (d2 + d3);
  sum = (s0 + s1) + (s2 + s3);
}
// sum_i v[i] w[i] and sum_i v[i] p[i] over two broadcast rows; the same additions in every lane
template <int CT>
__device__ __forceinline__ void dot_dot(const float* vrow, const float* prow, const float (&w)[CT], float& dw, float& dp) {
  const f4* v4 = reinterpret_cast<const f4*>(vrow);
  const f4* p4 = reinterpret_cast<const f4*>(prow);
  float d0 = 0.f, d1 = 0.f, d2 = 0.f, d3 = 0.f, s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
  for (int q = 0; q < CT / 4; ++q) {
    const f4 x = v4[q], p = p4[q];
    d0 = __builtin_fmaf(x.x, w[4 * q], d0);
    d1 = __builtin_fmaf(x.y, w[4 * q + 1], d1);
    d2 = __builtin_fmaf(x.z, w[4 * q + 2], d2);
    d3 = __builtin_fmaf(x.w, w[4 * q + 3], d3);
    s0 = __builtin_fmaf(x.x, p.x, s0);
    s1 = __builtin_fmaf(x.y, p.y, s1);
    s2 = __builtin_fmaf(x.z, p.z, s2);
    s3 = __builtin_fmaf(x.w, p.w, s3);
  }
  dw = (d0 + d1) + (d2 + d3);
  dp = (s0 + s1) + (s2 + s3);
}

// d[i] = sum_b grad[b] partial[b][i] in the order of b, overwritten or accumulated; partial[b] = [start C | end C | trans C*C].
// One thread per i: the body of lat_param_reduce_kernel and risk_param_reduce_kernel, which stay two kernels because their
// files differ in the contraction mode (s += grad * partial is one FMA under "fast", a product and a sum under "off").
__device__ __forceinline__ void param_reduce(const float* __restrict__ partial, const float* __restrict__ grad, int B, int C,
                                             float* __restrict__ dstart, float* __restrict__ dend, float* __restrict__ dtrans,
                                             int accumulate) {
  const int n = 2 * C + C * C;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float s = 0.f;
  for (int b = 0; b < B; ++b) s += grad[b] * partial[(long)b * n + i];
  float* d = i < C ? dstart + i : (i < 2 * C ? dend + (i - C) : dtrans + (i - 2 * C));
  if (accumulate) s += *d;
  *d = s;
}

// host side: the unrolled width CT of the lattice / risk / path kernels, and the shapes every chain kernel refuses
inline int width(int C) { return C <= 16 ? 16 : (C <= 32 ? 32 : 64); }
inline bool bad_shape(int B, int S, int C) {
  return B <= 0 || S < 1 || S > CRF_CHAIN_SMAX || C < 1 || C > CRF_CHAIN_CMAX;
}

// LAUNCH(CT) for CT = width(C)  (crf_wide.hip rounds C up to 32, 48 or 64 and keeps a rule of its own)
#define CRF_CHAIN_DISPATCH(C, LAUNCH) \
  switch (width(C)) {                 \
    case 16: LAUNCH(16); break;       \
    case 32: LAUNCH(32); break;       \
    default: LAUNCH(64); break;       \
  }

}  // namespace mtvaf
