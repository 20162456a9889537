// Token-level divergence between the emissions of two passes over the same batch: the consistency
// term of R-Drop (symmetric KL) and the textbook Jensen-Shannon divergence, per token, over up to 64 tags.
//
//   x, y [N,C] fp32, N = B*S rows; per live row  u = x/T, v = y/T, lp = log_softmax(u), lq = log_softmax(v), p = e^lp, q = e^lq
//   kind 0  L = 1/2 sum_c (p - q)(lp - lq)                                   dL/du = 1/2 [p (d - A) + p - q],  d = lp - lq, A = sum p d
//   kind 1  L = 1/2 sum_c p (lp - lm) + 1/2 sum_c q (lq - lm),  lm = log((p + q)/2)    dL/du = 1/2 p (a - Abar),  a = lp - lm, Abar = sum p a
//   loss = scale * (sum of L over live rows) / D,  D = live rows (counted here) or B
//
// Layout.  A row lives in a group of G lanes, lane = tag: G = 16 (four rows per wave) for C <= 16, G = 64 (one row per wave) above.
// Every row quantity (max, sum of exponentials, A, Abar, L) is a butterfly over the group's lanes; nothing of a row touches LDS.
// The work is latency-bound at the tagger's shapes (4096 x 11: 360 KB in, one group iteration per wave), so the kernels are
// written for few dependent steps, not for bandwidth.
//
// Log space.  lp and lq are finite for finite logits whatever their size; p and q may underflow to 0 and then multiply finite
// factors.  For the JS term  lp - lm = h - max(lq - lp, 0)  and  lq - lm = h + min(lq - lp, 0)  with
// h = -log1p(expm1(-|lq - lp|) / 2) in [0, log 2]: exact 0 for equal rows, no cancellation for close ones.
//
// Order.  The forward writes every row's L (0 on masked rows) to row_ws; one finishing block adds them in double, thread t the
// rows t, t + 1024, ... in rising order, then a fixed tree, and counts the live rows.  The partial sums are the rows
// themselves: row_ws is written anyway and no further scratch is needed.  The backward counts the live rows again in every block
// (an integer count over N mask bytes, 16 per load: 4 KB at the tagger's shape) instead of reading anything the forward left.
// No floating-point atomics anywhere.
#include <cmath>

#include "common.h"

namespace mtvaf {

constexpr int TD_THREADS = 256;    // row kernels: 4 waves, 256 / G rows per block and iteration
constexpr int TD_FINISH = 1024;    // the finishing block
constexpr int TD_MAX_BLOCKS = 2048;

template <int G>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, G);
  return v;
}
template <int G>
__device__ __forceinline__ float group_max(float v) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, G));
  return v;
}

// log_softmax of one row over the group's lanes; lanes at or past C carry u = -inf and return -inf (never used in a product).
template <int G>
__device__ __forceinline__ float group_log_softmax(float u) {
  const float m = group_max<G>(u);
  const float s = group_sum<G>(expf(u - m));  // the lane of the maximum adds 1: s >= 1
  return u - m - logf(s);
}

// bytes of w that are not 0
__device__ __forceinline__ int nonzero_bytes(uint32_t w) {
  return __popc((((w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | w) & 0x80808080u);
}

// Live rows of mask [N], by all NT threads of the block; every thread returns the count.  16-byte loads over the aligned body.
template <int NT>
__device__ __forceinline__ int block_count_live(const uint8_t* __restrict__ mask, int N, int* red) {
  const int tid = threadIdx.x;
  const int head = min(N, (int)((16 - ((uintptr_t)mask & 15)) & 15));
  const int n16 = (N - head) / 16, tail = head + n16 * 16;
  int cnt = 0;
  for (int i = tid; i < head; i += NT) cnt += mask[i] != 0;
  const uint4* m4 = reinterpret_cast<const uint4*>(mask + head);
  for (int i = tid; i < n16; i += NT) {
    const uint4 w = m4[i];
    cnt += nonzero_bytes(w.x) + nonzero_bytes(w.y) + nonzero_bytes(w.z) + nonzero_bytes(w.w);
  }
  for (int i = tail + tid; i < N; i += NT) cnt += mask[i] != 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if ((tid & 63) == 0) red[tid >> 6] = cnt;
  __syncthreads();
  int total = 0;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) total += red[w];
  return total;
}

// One row in its group: this lane's (lp, lq, p, q); lanes at or past C get act = false and zeros in p, q.
struct TdLane {
  float lp, lq, p, q;
  bool act;
};
template <int G>
__device__ __forceinline__ TdLane td_lane(const float* __restrict__ x, const float* __restrict__ y, long row, int C, int c,
                                          float inv_t) {
  TdLane k;
  k.act = c < C;
  const float u = k.act ? x[row * C + c] * inv_t : -INFINITY;
  const float v = k.act ? y[row * C + c] * inv_t : -INFINITY;
  k.lp = group_log_softmax<G>(u);
  k.lq = group_log_softmax<G>(v);
  k.p = k.act ? expf(k.lp) : 0.f;
  k.q = k.act ? expf(k.lq) : 0.f;
  return k;
}

// (a, b) = (lp - lm, lq - lm) of the JS term, see the file comment
__device__ __forceinline__ void js_logs(float lp, float lq, float& a, float& b) {
  const float dd = lq - lp;
  const float h = -log1pf(0.5f * expm1f(-fabsf(dd)));
  a = h - fmaxf(dd, 0.f);
  b = h + fminf(dd, 0.f);
}

template <int G, int KIND>
__global__ __launch_bounds__(TD_THREADS) void token_divergence_fwd_kernel(const float* __restrict__ x,
                                                                         const float* __restrict__ y,
                                                                         const uint8_t* __restrict__ mask,
                                                                         float* __restrict__ row_ws, int N, int C, float inv_t) {
  constexpr int RPB = TD_THREADS / G;
  const int c = threadIdx.x % G;
  for (long row = (long)blockIdx.x * RPB + threadIdx.x / G; row < N; row += (long)gridDim.x * RPB) {  // uniform per group
    float L = 0.f;
    if (!mask || mask[row]) {
      const TdLane k = td_lane<G>(x, y, row, C, c, inv_t);
      float t = 0.f;
      if (k.act) {
        if (KIND == 0) {
          t = (k.p - k.q) * (k.lp - k.lq);
        } else {
          float a, b;
          js_logs(k.lp, k.lq, a, b);
          t = k.p * a + k.q * b;
        }
      }
      L = 0.5f * group_sum<G>(t);
    }
    if (c == 0) row_ws[row] = L;
  }
}

// loss = scale * sum(row_ws) / D in double and in a fixed order; D = live rows (reduction 0) or B
__global__ __launch_bounds__(TD_FINISH) void token_divergence_finish_kernel(const float* __restrict__ row_ws,
                                                                           const uint8_t* __restrict__ mask,
                                                                           float* __restrict__ loss, int N, int reduction, int B,
                                                                           float scale) {
  __shared__ double red[TD_FINISH];
  __shared__ int cred[TD_FINISH / 64];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int i = tid; i < N; i += TD_FINISH) s += (double)row_ws[i];
  red[tid] = s;
  long D = B;
  if (reduction == 0) D = mask ? block_count_live<TD_FINISH>(mask, N, cred) : N;  // (uniform branch; its barrier also covers red)
  __syncthreads();
  for (int o = TD_FINISH / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) *loss = D > 0 ? (float)((double)scale * red[0] / (double)D) : 0.f;
}

template <int G, int KIND>
__global__ __launch_bounds__(TD_THREADS) void token_divergence_bwd_kernel(const float* __restrict__ gout,
                                                                         const float* __restrict__ x,
                                                                         const float* __restrict__ y,
                                                                         const uint8_t* __restrict__ mask, float* __restrict__ dx,
                                                                         float* __restrict__ dy, int N, int C, float inv_t,
                                                                         int reduction, int B, float scale) {
  constexpr int RPB = TD_THREADS / G;
  __shared__ int cred[TD_THREADS / 64];
  long D = B;
  if (reduction == 0) D = mask ? block_count_live<TD_THREADS>(mask, N, cred) : N;
  const float g = D > 0 ? 0.5f * *gout * scale * inv_t / (float)D : 0.f;  // 1/2 of both kinds, d/dx = d/du / T
  const int c = threadIdx.x % G;
  for (long row = (long)blockIdx.x * RPB + threadIdx.x / G; row < N; row += (long)gridDim.x * RPB) {
    float vx = 0.f, vy = 0.f;
    if (!mask || mask[row]) {
      const TdLane k = td_lane<G>(x, y, row, C, c, inv_t);
      if (KIND == 0) {
        const float d = k.lp - k.lq;
        const float A = group_sum<G>(k.act ? k.p * d : 0.f);
        const float Aq = group_sum<G>(k.act ? k.q * d : 0.f);  // = -sum q (lq - lp)
        if (k.act) {
          vx = g * (k.p * (d - A) + (k.p - k.q));
          vy = g * (k.q * (Aq - d) + (k.q - k.p));
        }
      } else {
        float a = 0.f, b = 0.f;
        if (k.act) js_logs(k.lp, k.lq, a, b);
        const float Ab = group_sum<G>(k.p * a);
        const float Bb = group_sum<G>(k.q * b);
        vx = g * k.p * (a - Ab);
        vy = g * k.q * (b - Bb);
      }
    }
    if (c < C) {
      dx[row * C + c] = vx;
      dy[row * C + c] = vy;
    }
  }
}

}  // namespace mtvaf

using namespace mtvaf;

static int td_check(const void* x, const void* y, int N, int C, int kind, float temperature, int reduction, int B) {
  if (N < 1 || C < 1 || C > 64) return MTVAF_ERR_SHAPE;
  if (!x || !y || (kind != 0 && kind != 1) || (reduction != 0 && reduction != 1) || !(temperature > 0.f) ||
      !std::isfinite(temperature) || (reduction == 1 && B < 1))
    return MTVAF_ERR_ARG;
  return MTVAF_OK;
}

static unsigned td_grid(int N, int G) {
  const int rpb = TD_THREADS / G;
  return (unsigned)std::min((N + rpb - 1) / rpb, TD_MAX_BLOCKS);
}

// Launches KERNEL<G, KIND> for the layout of C and the kind, over the rows N of the enclosing entry point, on its stream st
#define TD_DISPATCH(KERNEL, C, kind, ...)                                                              \
  do {                                                                                                 \
    if ((C) <= 16) {                                                                                   \
      if ((kind) == 0) hipLaunchKernelGGL((KERNEL<16, 0>), dim3(td_grid(N, 16)), dim3(TD_THREADS), 0, st, __VA_ARGS__); \
      else hipLaunchKernelGGL((KERNEL<16, 1>), dim3(td_grid(N, 16)), dim3(TD_THREADS), 0, st, __VA_ARGS__);             \
    } else {                                                                                           \
      if ((kind) == 0) hipLaunchKernelGGL((KERNEL<64, 0>), dim3(td_grid(N, 64)), dim3(TD_THREADS), 0, st, __VA_ARGS__); \
      else hipLaunchKernelGGL((KERNEL<64, 1>), dim3(td_grid(N, 64)), dim3(TD_THREADS), 0, st, __VA_ARGS__);             \
    }                                                                                                  \
  } while (0)

extern "C" {

int mtvaf_token_divergence_fwd(const float* x, const float* y, const uint8_t* mask, float* loss, float* row_ws, int N, int C,
                               int kind, float temperature, int reduction, int B, float scale, hipStream_t st) {
  const int rc = td_check(x, y, N, C, kind, temperature, reduction, B);
  if (rc != MTVAF_OK) return rc;
  if (!loss || !row_ws) return MTVAF_ERR_ARG;
  const float inv_t = 1.0f / temperature;
  TD_DISPATCH(token_divergence_fwd_kernel, C, kind, x, y, mask, row_ws, N, C, inv_t);
  hipLaunchKernelGGL(token_divergence_finish_kernel, dim3(1), dim3(TD_FINISH), 0, st, row_ws, mask, loss, N, reduction, B,
                     scale);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

int mtvaf_token_divergence_bwd(const float* grad_out, const float* x, const float* y, const uint8_t* mask, float* dx, float* dy,
                               int N, int C, int kind, float temperature, int reduction, int B, float scale, hipStream_t st) {
  const int rc = td_check(x, y, N, C, kind, temperature, reduction, B);
  if (rc != MTVAF_OK) return rc;
  if (!grad_out || !dx || !dy) return MTVAF_ERR_ARG;
  const float inv_t = 1.0f / temperature;
  TD_DISPATCH(token_divergence_bwd_kernel, C, kind, grad_out, x, y, mask, dx, dy, N, C, inv_t, reduction, B, scale);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

}  // extern "C"
