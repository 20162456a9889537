// Adversarial perturbation of the embedding output (FGM / PGD / FreeLB step; mtvaf_amd/adversarial.py -- new functionality, the
// reference trainer has no adversarial step).  g [B,S,H] is the gradient at the embedding output, mask [B,S] marks the live rows:
//
//   L2,   no delta_in   delta = eps * g / |g|_u                                   (FGM)
//   L2,   delta_in      d = delta_in + step * g / |g|_u ;  |d|_u > eps: d *= eps / |d|_u    (PGD / FreeLB: step, then project)
//   Linf, no delta_in   delta = eps * sign(g)
//   Linf, delta_in      delta = clamp(delta_in + step * sign(g), -eps, eps)
//
// u = all live rows of a sentence (scope sentence) or one live row (scope token).  Rows with mask 0 are never read from g / delta_in
// and get exact zeros; a unit whose norm is 0 or does not fit fp32 (inf, NaN) contributes no gradient term.
//
// Design: the ROW is the unit of work -- one wave holds a row (H <= 1024: 16 floats per lane) in registers, so a row is read once per
// launch and every block of the grid is busy (B*S/4 blocks: 1024 at the headline shape 32 x 128 x 768, against 32 for a block per
// sentence), and the sentence-wide sums go through a double workspace of one slot per row:
//
//   adv_sq_kernel       slot[row] = sum_h g^2, squares and sums in double from the first operation (as csrc/gradnorm.hip: a gradient
//                       of 1e-25 squares to 1e-50, which fp32 cannot hold)
//   adv_step_kernel<0>  only for L2 with delta_in: slot2[row] = sum_h d^2 of the stepped, unprojected d
//   adv_step_kernel<1>  forms d again from g and delta_in, projects, writes delta_out / out and slot3[row] = sum_h delta_out^2
//   adv_stats_kernel    stats[b] = {|g| over the live rows, |delta_out|}, one wave per sentence
//
// A wave that needs its sentence's sum adds the sentence's S slots itself, lane-strided and then by butterfly: every wave of a
// sentence adds the same numbers in the same order and gets the same bits.  No atomics, no host synchronisation: the same inputs give
// the same bits.  The fp32 arithmetic per element is: the norm rounded to fp32, one division, one multiplication (FGM) -- each
// commutes with a power-of-two scale of g, so g * 2^k gives bit-identical deltas.  out is formed from the ROUNDED delta by one
// addition that is kept from fusing with the product before it: out == x + delta_out bit for bit.
#include "common.h"

namespace mtvaf {

constexpr int ADV_MAX_S = 512, ADV_MAX_H = 1024;
constexpr int ADV_WAVES = 4;          // waves (= rows) per block
constexpr int ADV_PER_LANE = 16;      // ADV_MAX_H / 64
constexpr long ADV_MAX_GRID = 1L << 20;

__device__ __forceinline__ double wave_sum_d(double x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}

// A row in registers.  VEC: four float4 per lane, element (v*64 + lane)*4 + c (H % 4 == 0 and every base 16-byte aligned: the host
// checks); otherwise sixteen scalars, element j*64 + lane.  Elements past H read as 0 and are not stored.
template <bool VEC>
__device__ __forceinline__ void row_load(const float* __restrict__ p, int H, int lane, float (&v)[ADV_PER_LANE]) {
  if (VEC) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = (q * 64 + lane) * 4;
      f32x4 t = {0.f, 0.f, 0.f, 0.f};
      if (e < H) t = *reinterpret_cast<const f32x4*>(p + e);
      v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < ADV_PER_LANE; ++j) {
      const int e = j * 64 + lane;
      v[j] = e < H ? p[e] : 0.f;
    }
  }
}

template <bool VEC>
__device__ __forceinline__ void row_store(float* p, int H, int lane, const float (&v)[ADV_PER_LANE]) {
  if (VEC) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = (q * 64 + lane) * 4;
      if (e < H) *reinterpret_cast<f32x4*>(p + e) = f32x4{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
    }
  } else {
#pragma unroll
    for (int j = 0; j < ADV_PER_LANE; ++j) {
      const int e = j * 64 + lane;
      if (e < H) p[e] = v[j];
    }
  }
}

__device__ __forceinline__ double row_sumsq(const float (&v)[ADV_PER_LANE]) {
  double a = 0.0;
#pragma unroll
  for (int j = 0; j < ADV_PER_LANE; ++j) {
    const double d = (double)v[j];
    a = fma(d, d, a);
  }
  return wave_sum_d(a);
}

// sum of a unit's slots: the row's own (token) or the S slots of its sentence in a fixed order (dead rows hold 0.0)
__device__ __forceinline__ double unit_sumsq(const double* __restrict__ slots, long row, int S, int scope, int lane) {
  if (scope == MTVAF_ADV_SCOPE_TOKEN) return slots[row];
  const double* __restrict__ p = slots + (row / S) * S;
  double a = 0.0;
  for (int s = lane; s < S; s += 64) a += p[s];
  return wave_sum_d(a);
}

template <bool VEC>
__global__ __launch_bounds__(ADV_WAVES * 64) void adv_sq_kernel(const float* __restrict__ g, const uint8_t* __restrict__ mask,
                                                                double* __restrict__ gsq, long rows, int H) {
  const int lane = threadIdx.x & 63;
  for (long row = (long)blockIdx.x * ADV_WAVES + (threadIdx.x >> 6); row < rows; row += (long)gridDim.x * ADV_WAVES) {
    double s = 0.0;
    if (mask[row]) {  // (wave-uniform)
      float v[ADV_PER_LANE];
      row_load<VEC>(g + row * H, H, lane, v);
      s = row_sumsq(v);
    }
    if (lane == 0) gsq[row] = s;
  }
}

// FINAL = false: the sum of squares of the stepped d (L2 with delta_in only); FINAL = true: the whole update.
// delta_out may be delta_in: a row is read and written by one wave, and no wave reads another row's elements.
template <bool VEC, bool FINAL>
__global__ __launch_bounds__(ADV_WAVES * 64) void adv_step_kernel(const float* __restrict__ g, const float* delta_in,
                                                                  const float* __restrict__ x, const uint8_t* __restrict__ mask,
                                                                  const double* __restrict__ gsq, double* dsq, double* __restrict__ osq,
                                                                  float* delta_out, float* __restrict__ out, long rows, int S, int H,
                                                                  float eps, float step, int norm, int scope) {
  const int lane = threadIdx.x & 63;
  for (long row = (long)blockIdx.x * ADV_WAVES + (threadIdx.x >> 6); row < rows; row += (long)gridDim.x * ADV_WAVES) {
    float d[ADV_PER_LANE];
    const bool live = mask[row] != 0;
    if (!live) {
      if (!FINAL) {
        if (lane == 0) dsq[row] = 0.0;
        continue;
      }
#pragma unroll
      for (int j = 0; j < ADV_PER_LANE; ++j) d[j] = 0.f;
    } else {
      const float ng = (float)sqrt(unit_sumsq(gsq, row, S, scope, lane));
      const bool ok = ng > 0.f && (ng - ng) == 0.f;  // a norm of 0, or one that fp32 cannot hold: the unit gets no gradient term
      float gv[ADV_PER_LANE], dv[ADV_PER_LANE];
      if (ok) {
        row_load<VEC>(g + row * H, H, lane, gv);
      } else {
#pragma unroll
        for (int j = 0; j < ADV_PER_LANE; ++j) gv[j] = 0.f;
      }
      if (delta_in) row_load<VEC>(delta_in + row * H, H, lane, dv);
#pragma unroll
      for (int j = 0; j < ADV_PER_LANE; ++j) {
        float t;  // the unit direction: g / |g|_u, or sign(g)
        if (norm == MTVAF_ADV_NORM_L2) t = ok ? __fdiv_rn(gv[j], ng) : 0.f;
        else t = gv[j] > 0.f ? 1.f : (gv[j] < 0.f ? -1.f : 0.f);
        if (delta_in) {
          d[j] = dv[j] + step * t;
          if (norm == MTVAF_ADV_NORM_LINF) d[j] = fminf(fmaxf(d[j], -eps), eps);
        } else {
          d[j] = __fmul_rn(eps, t);
        }
      }
      if (norm == MTVAF_ADV_NORM_L2 && delta_in) {
        if (!FINAL) {
          const double s = row_sumsq(d);
          if (lane == 0) dsq[row] = s;
          continue;
        }
        const float nd = (float)sqrt(unit_sumsq(dsq, row, S, scope, lane));
        if (nd > eps) {
          const float c = __fdiv_rn(eps, nd);
#pragma unroll
          for (int j = 0; j < ADV_PER_LANE; ++j) d[j] = __fmul_rn(d[j], c);
        }
      }
    }
    if (FINAL) {
      row_store<VEC>(delta_out + row * H, H, lane, d);
      const double s = live ? row_sumsq(d) : 0.0;
      if (lane == 0) osq[row] = s;
      if (out) {
        float xv[ADV_PER_LANE];
        row_load<VEC>(x + row * H, H, lane, xv);
#pragma unroll
        for (int j = 0; j < ADV_PER_LANE; ++j) xv[j] = __fadd_rn(xv[j], d[j]);  // (never fused with the product that made d)
        row_store<VEC>(out + row * H, H, lane, xv);
      }
    }
  }
}

__global__ __launch_bounds__(ADV_WAVES * 64) void adv_stats_kernel(const double* __restrict__ gsq, const double* __restrict__ osq,
                                                                   float* __restrict__ stats, long B, int S) {
  const int lane = threadIdx.x & 63;
  for (long b = (long)blockIdx.x * ADV_WAVES + (threadIdx.x >> 6); b < B; b += (long)gridDim.x * ADV_WAVES) {
    const double sg = unit_sumsq(gsq, b * S, S, MTVAF_ADV_SCOPE_SENTENCE, lane);
    const double so = unit_sumsq(osq, b * S, S, MTVAF_ADV_SCOPE_SENTENCE, lane);
    if (lane == 0) {
      stats[2 * b] = (float)sqrt(sg);
      stats[2 * b + 1] = (float)sqrt(so);
    }
  }
}

__global__ __launch_bounds__(256) void adv_add_kernel(const float* __restrict__ x, const float* __restrict__ d, float* __restrict__ out,
                                                      long n, long n4) {
  const long stride = (long)gridDim.x * 256;
  const f32x4* __restrict__ x4 = reinterpret_cast<const f32x4*>(x);
  const f32x4* __restrict__ d4 = reinterpret_cast<const f32x4*>(d);
  f32x4* __restrict__ o4 = reinterpret_cast<f32x4*>(out);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) o4[i] = x4[i] + d4[i];
  for (long i = (n4 << 2) + (long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) out[i] = x[i] + d[i];  // scalar tail
}

static inline unsigned adv_grid(long items) {
  const long blocks = (items + ADV_WAVES - 1) / ADV_WAVES;
  return (unsigned)(blocks < ADV_MAX_GRID ? blocks : ADV_MAX_GRID);
}

template <bool VEC>
static int adv_launch(const float* g, const float* delta_in, const float* x, const uint8_t* mask, float* delta_out, float* out,
                      float* stats, long B, int S, int H, float eps, float step, int norm, int scope, double* ws, hipStream_t st) {
  const long rows = B * S;
  double *gsq = ws, *dsq = ws + rows, *osq = ws + 2 * rows;
  const dim3 grid(adv_grid(rows)), block(ADV_WAVES * 64);
  hipLaunchKernelGGL(adv_sq_kernel<VEC>, grid, block, 0, st, g, mask, gsq, rows, H);
  MTVAF_LAUNCH_CHECK();
  if (norm == MTVAF_ADV_NORM_L2 && delta_in) {
    hipLaunchKernelGGL((adv_step_kernel<VEC, false>), grid, block, 0, st, g, delta_in, x, mask, gsq, dsq, osq, delta_out, out, rows,
                       S, H, eps, step, norm, scope);
    MTVAF_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL((adv_step_kernel<VEC, true>), grid, block, 0, st, g, delta_in, x, mask, gsq, dsq, osq, delta_out, out, rows, S,
                     H, eps, step, norm, scope);
  MTVAF_LAUNCH_CHECK();
  hipLaunchKernelGGL(adv_stats_kernel, dim3(adv_grid(B)), block, 0, st, gsq, osq, stats, B, S);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

}  // namespace mtvaf

using namespace mtvaf;

extern "C" {

// bytes of the workspace of mtvaf_adv_perturb: three doubles per row (sums of squares of g, of the stepped d, of delta_out).
// 0 for a bad argument (the call itself reports it).
size_t mtvaf_adv_workspace_bytes(int B, int S) {
  if (B < 1 || S < 1 || S > ADV_MAX_S) return 0;
  return (size_t)B * (size_t)S * 3 * sizeof(double);
}

int mtvaf_adv_perturb(const float* g, const float* delta_in, const float* x, const uint8_t* mask, float* delta_out, float* out,
                      float* stats, int B, int S, int H, float eps, float step, int norm, int scope, void* ws, size_t ws_bytes,
                      hipStream_t stream) {
  if (B < 1 || S < 1 || S > ADV_MAX_S || H < 1 || H > ADV_MAX_H) return MTVAF_ERR_SHAPE;
  if (!g || !mask || !delta_out || !stats || !ws || (out && !x)) return MTVAF_ERR_ARG;
  if ((norm != MTVAF_ADV_NORM_L2 && norm != MTVAF_ADV_NORM_LINF) || (scope != MTVAF_ADV_SCOPE_SENTENCE && scope != MTVAF_ADV_SCOPE_TOKEN))
    return MTVAF_ERR_ARG;
  if (!(eps >= 0.f) || !(step >= 0.f) || (eps - eps) != 0.f || (step - step) != 0.f) return MTVAF_ERR_ARG;  // (NaN, inf, negative)
  const uintptr_t all = (uintptr_t)g | (uintptr_t)delta_in | (uintptr_t)x | (uintptr_t)delta_out | (uintptr_t)out;
  if ((all & 3) || ((uintptr_t)stats & 3) || ((uintptr_t)ws & 7)) return MTVAF_ERR_ALIGN;
  if (ws_bytes < mtvaf_adv_workspace_bytes(B, S)) return MTVAF_ERR_WORKSPACE;
  const bool vec = (H & 3) == 0 && (all & 15) == 0;
  return vec ? adv_launch<true>(g, delta_in, x, mask, delta_out, out, stats, B, S, H, eps, step, norm, scope, static_cast<double*>(ws), stream)
             : adv_launch<false>(g, delta_in, x, mask, delta_out, out, stats, B, S, H, eps, step, norm, scope, static_cast<double*>(ws), stream);
}

int mtvaf_adv_add(const float* x, const float* delta, float* out, long n, hipStream_t stream) {
  if (!x || !delta || !out || n < 1) return MTVAF_ERR_ARG;
  const uintptr_t all = (uintptr_t)x | (uintptr_t)delta | (uintptr_t)out;
  if (all & 3) return MTVAF_ERR_ALIGN;
  const long n4 = (all & 15) == 0 ? (n >> 2) : 0;
  const long blocks = (((n4 ? n4 : n) + 255) / 256);
  hipLaunchKernelGGL(adv_add_kernel, dim3((unsigned)(blocks < 2048 ? (blocks ? blocks : 1) : 2048)), dim3(256), 0, stream, x, delta, out, n, n4);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

}  // extern "C"
