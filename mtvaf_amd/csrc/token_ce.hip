// Token-level cross entropy over the tagger's emissions: the loss of a softmax tagging head and the
// auxiliary term beside the CRF -- class weights, label smoothing and the focal factor in one row pass -- and the per-token
// first maximum with its log-probability for decoding.
//
//   logits [N,C] fp32, labels [N] int64, mask [N] u8 or NULL, class_weight w [C] or NULL (all ones)
//   live row: mask byte non-zero (or no mask), label != ignore_index, 0 <= label < C
//   per live row, y = label, lp = log_softmax(z), p = e^lp, eps = smoothing, g = gamma:
//     a_c = (1 - eps) w_y [c = y] + (eps / C) w_c        A = sum_c a_c
//     ce  = -sum_c a_c lp_c         om = sum_{c != y} p_c         L = om^g ce   (g = 0: L = ce)
//     dL/dz_k = om^g (A p_k - a_k) - ce g om^(g-1) p_y ([k = y] - p_k)
//   loss = scale * (sum of L over live rows) / D,   D = sum_live w_y (0) | B (1) | 1 (2)
//
// Layout as in consistency.hip: a row lives in a group of G lanes, lane = tag, G = 16 (four rows per wave) for C <= 16 and
// G = 64 above; every row quantity is a butterfly over the group's lanes and the independent ones (A, ce, om) run side by side.
// The work is latency-bound at the tagger's shapes (4096 x 11: 180 KB in), so the kernels are written for few dependent steps.
//
// om is formed as the sum of the OTHER tags' probabilities, never as 1 - p_y: it keeps its relative accuracy as p_y -> 1, and it
// is exactly 0 when every other tag underflows, so the focal value and gradient of such a row are exact zeros.  [k = y] - p_k at
// k = y is that same om.  lp is finite for finite logits whatever their size; a_c = 0 multiplies a finite lp_c.
//
// Order.  The forward writes every row's L (0 on dead rows) to row_ws; one finishing block adds the rows and D in double,
// thread t the rows t, t + 1024, ... in rising order, then a fixed tree, and counts the live rows and the out-of-range labels
// into stats.  The backward forms D again in every block, in double and in a fixed order (N labels: 32 KB at the tagger's shape,
// read only by the 'mean' reduction), instead of reading anything the forward left.  No floating-point atomics anywhere.
#include <cmath>

#include "common.h"

namespace mtvaf {

constexpr int TC_THREADS = 256;    // row kernels: 4 waves, 256 / G rows per block and iteration
constexpr int TC_FINISH = 1024;    // the finishing block
constexpr int TC_MAX_BLOCKS = 2048;

template <int G>
__device__ __forceinline__ float tc_sum(float v) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, G);
  return v;
}
template <int G>
__device__ __forceinline__ float tc_max(float v) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, G));
  return v;
}

// 0: dead (masked or ignore_index), 1: live, 2: dead with a label outside [0, C) that is not ignore_index.  The label of a
// masked row is not looked at.
__device__ __forceinline__ int tc_row_state(const int64_t* __restrict__ labels, const uint8_t* __restrict__ mask, long row, int C,
                                            int64_t ignore_index, int& y) {
  y = 0;
  if (mask && !mask[row]) return 0;
  const int64_t l = labels[row];
  if (l == ignore_index) return 0;
  if (l < 0 || l >= C) return 2;
  y = (int)l;
  return 1;
}

// One live row in its group.  Every lane gets the row's ce, om, A and p_y; its own p and a (zeros at or past C).
struct TcRow {
  float p, a, ce, om, A, py;
};
template <int G>
__device__ __forceinline__ TcRow tc_row(const float* __restrict__ logits, const float* __restrict__ cw, long row, int C, int c, int y,
                                        float smoothing) {
  const bool act = c < C;
  const float z = act ? logits[row * C + c] : -INFINITY;
  const float wc = act ? (cw ? cw[c] : 1.f) : 0.f;
  const float wy = cw ? cw[y] : 1.f;
  const float m = tc_max<G>(z);
  const float e = act ? expf(z - m) : 0.f;
  const float s = tc_sum<G>(e);  // the lane of the maximum adds 1: s >= 1
  const float lp = z - m - logf(s);
  TcRow r;
  r.p = act ? expf(lp) : 0.f;
  r.a = (c == y ? (1.f - smoothing) * wy : 0.f) + (smoothing / (float)C) * wc;
  // three independent butterflies
  float ce = act ? -r.a * lp : 0.f, om = c == y ? 0.f : r.p, A = r.a;
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) {
    ce += __shfl_xor(ce, o, G);
    om += __shfl_xor(om, o, G);
    A += __shfl_xor(A, o, G);
  }
  r.ce = ce, r.om = om, r.A = A;
  r.py = __shfl(r.p, y, G);
  return r;
}

template <int G>
__global__ __launch_bounds__(TC_THREADS) void token_ce_fwd_kernel(const float* __restrict__ logits,
                                                                 const int64_t* __restrict__ labels,
                                                                 const uint8_t* __restrict__ mask, const float* __restrict__ cw,
                                                                 float* __restrict__ row_ws, int N, int C, long ignore_index,
                                                                 float smoothing, float gamma) {
  constexpr int RPB = TC_THREADS / G;
  const int c = threadIdx.x % G;
  for (long row = (long)blockIdx.x * RPB + threadIdx.x / G; row < N; row += (long)gridDim.x * RPB) {  // uniform per group
    float L = 0.f;
    int y;
    if (tc_row_state(labels, mask, row, C, ignore_index, y) == 1) {
      const TcRow r = tc_row<G>(logits, cw, row, C, c, y, smoothing);
      L = gamma == 0.f ? r.ce : powf(r.om, gamma) * r.ce;
    }
    if (c == 0) row_ws[row] = L;
  }
}

// (sum of row_ws, D, live rows, out-of-range labels) over all rows by the NT threads of a block, in double and in a fixed order:
// thread t the rows t, t + NT, ... rising, then a tree.  rows may be NULL (the backward needs D only).
template <int NT>
__device__ __forceinline__ void tc_block_totals(const float* __restrict__ rows, const int64_t* __restrict__ labels,
                                                const uint8_t* __restrict__ mask, const float* __restrict__ cw, int N, int C,
                                                int64_t ignore_index, double* red_s, double* red_d, int* red_n, double& S,
                                                double& D, int& n_live, int& n_bad) {
  const int tid = threadIdx.x;
  double s = 0.0, d = 0.0;
  int live = 0, bad = 0;
  for (int i = tid; i < N; i += NT) {
    int y;
    const int st = tc_row_state(labels, mask, i, C, ignore_index, y);
    if (rows) s += (double)rows[i];
    if (st == 1) {
      d += cw ? (double)cw[y] : 1.0;
      ++live;
    }
    bad += st == 2;
  }
  red_s[tid] = s, red_d[tid] = d, red_n[tid] = live, red_n[NT + tid] = bad;
  __syncthreads();
  for (int o = NT / 2; o > 0; o >>= 1) {
    if (tid < o) {
      red_s[tid] += red_s[tid + o];
      red_d[tid] += red_d[tid + o];
      red_n[tid] += red_n[tid + o];
      red_n[NT + tid] += red_n[NT + tid + o];
    }
    __syncthreads();
  }
  S = red_s[0], D = red_d[0], n_live = red_n[0], n_bad = red_n[NT];
}

__global__ __launch_bounds__(TC_FINISH) void token_ce_finish_kernel(const float* __restrict__ row_ws,
                                                                   const int64_t* __restrict__ labels,
                                                                   const uint8_t* __restrict__ mask, const float* __restrict__ cw,
                                                                   float* __restrict__ loss, int* __restrict__ stats, int N, int C,
                                                                   int64_t ignore_index, int reduction, int B, float scale) {
  __shared__ double red_s[TC_FINISH], red_d[TC_FINISH];
  __shared__ int red_n[2 * TC_FINISH];
  double S, D;
  int n_live, n_bad;
  tc_block_totals<TC_FINISH>(row_ws, labels, mask, cw, N, C, ignore_index, red_s, red_d, red_n, S, D, n_live, n_bad);
  if (reduction == 1) D = (double)B;
  if (reduction == 2) D = 1.0;
  if (threadIdx.x == 0) {
    *loss = D > 0.0 ? (float)((double)scale * S / D) : 0.f;
    stats[0] = n_live;
    stats[1] = n_bad;
  }
}

template <int G>
__global__ __launch_bounds__(TC_THREADS) void token_ce_bwd_kernel(const float* __restrict__ gout, const float* __restrict__ grows,
                                                                 const float* __restrict__ logits,
                                                                 const int64_t* __restrict__ labels,
                                                                 const uint8_t* __restrict__ mask, const float* __restrict__ cw,
                                                                 float* __restrict__ dlogits, int N, int C, long ignore_index,
                                                                 float smoothing, float gamma, int reduction, int B, float scale) {
  constexpr int RPB = TC_THREADS / G;
  __shared__ double red_s[TC_THREADS], red_d[TC_THREADS];
  __shared__ int red_n[2 * TC_THREADS];
  float g = scale;  // per-row upstream: scale * grad_rows[row]
  if (!grows) {
    double D = reduction == 1 ? (double)B : 1.0;
    if (reduction == 0) {  // (uniform branch)
      double S;
      int n_live, n_bad;
      tc_block_totals<TC_THREADS>(nullptr, labels, mask, cw, N, C, ignore_index, red_s, red_d, red_n, S, D, n_live, n_bad);
    }
    g = D > 0.0 ? (float)((double)*gout * (double)scale / D) : 0.f;
  }
  const int c = threadIdx.x % G;
  for (long row = (long)blockIdx.x * RPB + threadIdx.x / G; row < N; row += (long)gridDim.x * RPB) {
    float v = 0.f;
    int y;
    if (tc_row_state(labels, mask, row, C, ignore_index, y) == 1) {
      const TcRow r = tc_row<G>(logits, cw, row, C, c, y, smoothing);
      const float gr = grows ? g * grows[row] : g;
      const float dce = r.A * r.p - r.a;
      if (gamma == 0.f) {
        v = gr * dce;
      } else {
        const float f1 = powf(r.om, gamma - 1.f);  // om^0 = 1 at om = 0
        v = gr * (f1 * r.om * dce - r.ce * gamma * f1 * r.py * (c == y ? r.om : -r.p));
      }
    }
    if (c < C) dlogits[row * C + c] = v;
  }
}

// First maximum of every live row over the permitted tags, and log_softmax (over all C tags) at it.
template <int G>
__global__ __launch_bounds__(TC_THREADS) void token_argmax_kernel(const float* __restrict__ logits, const uint8_t* __restrict__ mask,
                                                                 const int64_t* __restrict__ allowed, int64_t* __restrict__ tags,
                                                                 float* __restrict__ logp, int N, int C) {
  constexpr int RPB = TC_THREADS / G;
  const int c = threadIdx.x % G;
  const uint64_t low = C == 64 ? ~0ull : (1ull << C) - 1ull;
  for (long row = (long)blockIdx.x * RPB + threadIdx.x / G; row < N; row += (long)gridDim.x * RPB) {
    int best = 0;
    float lp = 0.f;
    if (!mask || mask[row]) {
      uint64_t set = allowed ? (uint64_t)allowed[row] & low : 0ull;
      if (set == 0ull) set = low;  // no constraint
      const bool act = c < C;
      const float z = act ? logits[row * C + c] : -INFINITY;
      const float m = tc_max<G>(z);
      const float s = tc_sum<G>(act ? expf(z - m) : 0.f);
      float bz = act && ((set >> c) & 1ull) ? z : -INFINITY;
      best = c;
#pragma unroll
      for (int o = G / 2; o > 0; o >>= 1) {
        const float oz = __shfl_xor(bz, o, G);
        const int oi = __shfl_xor(best, o, G);
        if (oz > bz || (oz == bz && oi < best)) bz = oz, best = oi;
      }
      lp = bz - m - logf(s);
    }
    if (c == 0) {
      tags[row] = best;
      logp[row] = lp;
    }
  }
}

}  // namespace mtvaf

using namespace mtvaf;

static int tc_check(const void* logits, const void* labels, int N, int C, float smoothing, float gamma, int reduction, int B) {
  if (N < 1 || C < 1 || C > 64) return MTVAF_ERR_SHAPE;
  if (!logits || !labels || !(smoothing >= 0.f && smoothing < 1.f) || !(gamma == 0.f || (gamma >= 1.f && gamma <= 8.f)) ||
      reduction < 0 || reduction > 2 || (reduction == 1 && B < 1))
    return MTVAF_ERR_ARG;
  return MTVAF_OK;
}

static unsigned tc_grid(int N, int G) {
  const int rpb = TC_THREADS / G;
  return (unsigned)std::min((N + rpb - 1) / rpb, TC_MAX_BLOCKS);
}

// Launches KERNEL<G> for the layout of C over the rows N of the enclosing entry point, on its stream st
#define TC_DISPATCH(KERNEL, C, ...)                                                                              \
  do {                                                                                                           \
    if ((C) <= 16) hipLaunchKernelGGL((KERNEL<16>), dim3(tc_grid(N, 16)), dim3(TC_THREADS), 0, st, __VA_ARGS__); \
    else hipLaunchKernelGGL((KERNEL<64>), dim3(tc_grid(N, 64)), dim3(TC_THREADS), 0, st, __VA_ARGS__);           \
  } while (0)

extern "C" {

int mtvaf_token_ce_fwd(const float* logits, const int64_t* labels, const uint8_t* mask, const float* class_weight, float* loss,
                       float* row_ws, int* stats, int N, int C, long ignore_index, float smoothing, float gamma, int reduction,
                       int B, float scale, hipStream_t st) {
  const int rc = tc_check(logits, labels, N, C, smoothing, gamma, reduction, B);
  if (rc != MTVAF_OK) return rc;
  if (!loss || !row_ws || !stats) return MTVAF_ERR_ARG;
  TC_DISPATCH(token_ce_fwd_kernel, C, logits, labels, mask, class_weight, row_ws, N, C, ignore_index, smoothing, gamma);
  hipLaunchKernelGGL(token_ce_finish_kernel, dim3(1), dim3(TC_FINISH), 0, st, row_ws, labels, mask, class_weight, loss, stats, N,
                     C, ignore_index, reduction, B, scale);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

int mtvaf_token_ce_bwd(const float* grad_out, const float* grad_rows, const float* logits, const int64_t* labels,
                       const uint8_t* mask, const float* class_weight, float* dlogits, int N, int C, long ignore_index,
                       float smoothing, float gamma, int reduction, int B, float scale, hipStream_t st) {
  const int rc = tc_check(logits, labels, N, C, smoothing, gamma, reduction, B);
  if (rc != MTVAF_OK) return rc;
  if (!dlogits || (grad_out == nullptr) == (grad_rows == nullptr)) return MTVAF_ERR_ARG;  // exactly one upstream gradient
  TC_DISPATCH(token_ce_bwd_kernel, C, grad_out, grad_rows, logits, labels, mask, class_weight, dlogits, N, C, ignore_index,
              smoothing, gamma, reduction, B, scale);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

int mtvaf_token_argmax(const float* logits, const uint8_t* mask, const int64_t* allowed, int64_t* tags, float* logp, int N, int C,
                       hipStream_t st) {
  if (N < 1 || C < 1 || C > 64) return MTVAF_ERR_SHAPE;
  if (!logits || !tags || !logp) return MTVAF_ERR_ARG;
  TC_DISPATCH(token_argmax_kernel, C, logits, mask, allowed, tags, logp, N, C);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

}  // extern "C"
