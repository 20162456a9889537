// Word-level tagging head (mtvaf_amd/words.py; new functionality, the reference tags word pieces): the word axis of a batch, the
// pooling of piece vectors onto it, and the pooling's backward.  DESIGN.md section 4.25.
//
//   mtvaf_word_index     attention_mask [B,S] u8 (a prefix mask), token_to_word [B,S] i32 (-1 outside the map) -> the columns.
//                        len = the leading non-zero entries of the mask.  Token s < len OPENS a column iff s == 0, map[s] < 0 or
//                        map[s] != map[s-1]: unmapped tokens ([CLS], [SEP]) are columns of their own, adjacent tokens with one
//                        non-negative map value are one column.  Integers only.  One wave per sentence, 64 tokens at a time: the
//                        column of a token is a prefix count of the "opens" ballot, the start of its column the highest set bit at
//                        or below its lane (or the carry of the chunks before), and the token that CLOSES a column (the next one
//                        opens, or it is the last live one) writes that column's start, length and word id.  Map entries at
//                        masked tokens are never read.
//   mtvaf_word_pool_fwd  x [B,S,H] -> y [B,W,H]: first piece, last piece, or the mean -- the pieces added one after the other in
//                        ascending token order, then ONE division by (float)col_len.  One wave per output row.
//   mtvaf_word_pool_bwd  dy [B,W,H] -> dx [B,S,H], a GATHER: one wave per token row reads its column's dy.
//
// Every element of every output is written by exactly one lane; no atomics, no LDS, no host synchronisation: the same inputs give
// the same bits.  x at masked tokens and dy at dead columns are never read.  The row kernels trust no index: a column or a token
// whose start / length / column does not lie inside the tensors is treated as dead (zeros), never followed.
#include "common.h"

namespace mtvaf {

constexpr int WP_MAX_S = 512;
constexpr int WP_WAVES = 4;  // waves per block: one sentence (index) or one row (pooling) each
constexpr long WP_MAX_GRID = 1L << 20;

__global__ __launch_bounds__(WP_WAVES * 64) void word_index_kernel(const uint8_t* __restrict__ mask, const int* __restrict__ map,
                                                                   int* __restrict__ col_start, int* __restrict__ col_len,
                                                                   int* __restrict__ col_of_token, uint8_t* __restrict__ word_mask,
                                                                   int* __restrict__ word_id, int* __restrict__ n_cols, long B,
                                                                   int S, int W) {
  const int lane = threadIdx.x & 63;
  const int chunks = (S + 63) >> 6;
  for (long b = (long)blockIdx.x * WP_WAVES + (threadIdx.x >> 6); b < B; b += (long)gridDim.x * WP_WAVES) {
    const uint8_t* __restrict__ mk = mask + b * S;
    const int* __restrict__ mp = map + b * S;
    int len = 0;  // the leading run of the mask (wave-uniform)
    for (int c = 0; c < chunks; ++c) {
      const int s = c * 64 + lane;
      const unsigned long long live = __ballot(s < S && mk[s] != 0);
      const int lead = ~live == 0ull ? 64 : __builtin_ctzll(~live);
      len += lead;
      if (lead < 64) break;
    }
    int base = 0;    // columns opened in the chunks before this one
    int carry = 0;   // first token of the last column opened so far
    for (int c = 0; c < chunks; ++c) {
      const int s = c * 64 + lane;
      const bool in = s < len;
      const int m = in ? mp[s] : -1;
      const int prev = (in && s > 0) ? mp[s - 1] : -1;
      const int next = (s + 1 < len) ? mp[s + 1] : -1;
      const bool opens = in && (s == 0 || m < 0 || m != prev);
      const bool closes = in && (s + 1 == len || next < 0 || next != m);
      const unsigned long long ob = __ballot(opens);
      const unsigned long long upto = ob & ((2ull << lane) - 1ull);  // opens at or below this lane (lane 63: all of them)
      const int col = base + __popcll(upto) - 1;
      const int start = upto ? c * 64 + 63 - __builtin_clzll(upto) : carry;
      if (s < S) col_of_token[b * S + s] = (in && col < W) ? col : -1;
      if (closes && col < W) {
        const long o = b * W + col;
        col_start[o] = start;
        col_len[o] = s - start + 1;
        word_id[o] = m < 0 ? -1 : m;
        word_mask[o] = 1;
      }
      base += __popcll(ob);
      if (ob) carry = c * 64 + 63 - __builtin_clzll(ob);
    }
    for (int w = (base < W ? base : W) + lane; w < W; w += 64) {  // dead columns
      const long o = b * W + w;
      col_start[o] = 0;
      col_len[o] = 0;
      word_id[o] = -1;
      word_mask[o] = 0;
    }
    if (lane == 0) n_cols[b] = base;
  }
}

// The arithmetic of the mean, stated once: additions in the order given, one correctly rounded division.  No reciprocal, and
// nothing here may be contracted or re-associated: the bits follow from this text.
__device__ __forceinline__ float wp_add(float a, float b) {
#pragma clang fp contract(off)
  return __fadd_rn(a, b);
}
__device__ __forceinline__ float wp_div(float a, float n) {
#pragma clang fp contract(off)
  return __fdiv_rn(a, n);
}

// One element group of a row: a float4 (VEC: H % 4 == 0 and every base 16-byte aligned, the host checks) or one float.
template <bool VEC> struct WpElem;
template <> struct WpElem<true> {
  typedef f32x4 T;
  static __device__ __forceinline__ int count(int H) { return H >> 2; }
  static __device__ __forceinline__ T load(const float* p, int i) { return reinterpret_cast<const f32x4*>(p)[i]; }
  static __device__ __forceinline__ void store(float* p, int i, T v) { reinterpret_cast<f32x4*>(p)[i] = v; }
  static __device__ __forceinline__ T zero() { return f32x4{0.f, 0.f, 0.f, 0.f}; }
  static __device__ __forceinline__ T add(T a, T b) { return f32x4{wp_add(a.x, b.x), wp_add(a.y, b.y), wp_add(a.z, b.z), wp_add(a.w, b.w)}; }
  static __device__ __forceinline__ T div(T a, float n) { return f32x4{wp_div(a.x, n), wp_div(a.y, n), wp_div(a.z, n), wp_div(a.w, n)}; }
};
template <> struct WpElem<false> {
  typedef float T;
  static __device__ __forceinline__ int count(int H) { return H; }
  static __device__ __forceinline__ T load(const float* p, int i) { return p[i]; }
  static __device__ __forceinline__ void store(float* p, int i, T v) { p[i] = v; }
  static __device__ __forceinline__ T zero() { return 0.f; }
  static __device__ __forceinline__ T add(T a, T b) { return wp_add(a, b); }
  static __device__ __forceinline__ T div(T a, float n) { return wp_div(a, n); }
};

template <bool VEC>
__global__ __launch_bounds__(WP_WAVES * 64) void word_pool_fwd_kernel(const float* __restrict__ x, const int* __restrict__ col_start,
                                                                      const int* __restrict__ col_len, float* __restrict__ y,
                                                                      long rows, int S, int W, int H, int mode) {
  typedef WpElem<VEC> E;
  const int lane = threadIdx.x & 63;
  const int n = E::count(H);
  for (long row = (long)blockIdx.x * WP_WAVES + (threadIdx.x >> 6); row < rows; row += (long)gridDim.x * WP_WAVES) {
    const int start = col_start[row], len = col_len[row];  // (wave-uniform)
    float* yr = y + row * H;
    if (len <= 0 || start < 0 || start > S - len) {  // a dead column (or an index that points outside the sentence)
      for (int i = lane; i < n; i += 64) E::store(yr, i, E::zero());
      continue;
    }
    const float* __restrict__ xs = x + ((row / W) * S + start) * H;
    if (mode == MTVAF_WORD_POOL_MEAN && len > 1) {
      const float fl = (float)len;
      for (int i = lane; i < n; i += 64) {
        typename E::T a = E::load(xs, i);
        for (int k = 1; k < len; ++k) a = E::add(a, E::load(xs + (long)k * H, i));
        E::store(yr, i, E::div(a, fl));
      }
    } else {  // first, last, and the mean of one piece (x / 1.0f is x): copies
      const float* __restrict__ src = mode == MTVAF_WORD_POOL_LAST ? xs + (long)(len - 1) * H : xs;
      for (int i = lane; i < n; i += 64) E::store(yr, i, E::load(src, i));
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(WP_WAVES * 64) void word_pool_bwd_kernel(const float* __restrict__ dy, const int* __restrict__ col_start,
                                                                      const int* __restrict__ col_len,
                                                                      const int* __restrict__ col_of_token, float* __restrict__ dx,
                                                                      long rows, int S, int W, int H, int mode) {
  typedef WpElem<VEC> E;
  const int lane = threadIdx.x & 63;
  const int n = E::count(H);
  for (long row = (long)blockIdx.x * WP_WAVES + (threadIdx.x >> 6); row < rows; row += (long)gridDim.x * WP_WAVES) {
    const long b = row / S;
    const int s = (int)(row - b * S);
    const int col = col_of_token[row];  // (wave-uniform)
    float* dr = dx + row * H;
    bool take = false;
    int len = 0;
    if (col >= 0 && col < W) {
      const int start = col_start[b * W + col];
      len = col_len[b * W + col];
      if (len > 0 && s >= start && s - start < len)
        take = mode == MTVAF_WORD_POOL_MEAN || (mode == MTVAF_WORD_POOL_FIRST ? s == start : s - start == len - 1);
    }
    if (!take) {  // masked, beyond W, or not the selected piece
      for (int i = lane; i < n; i += 64) E::store(dr, i, E::zero());
      continue;
    }
    const float* __restrict__ src = dy + (b * W + col) * H;
    if (mode == MTVAF_WORD_POOL_MEAN && len > 1) {
      const float fl = (float)len;
      for (int i = lane; i < n; i += 64) E::store(dr, i, E::div(E::load(src, i), fl));
    } else {
      for (int i = lane; i < n; i += 64) E::store(dr, i, E::load(src, i));
    }
  }
}

static inline unsigned wp_grid(long items) {
  const long blocks = (items + WP_WAVES - 1) / WP_WAVES;
  return (unsigned)(blocks < WP_MAX_GRID ? blocks : WP_MAX_GRID);
}

static inline bool wp_mode_ok(int mode) {
  return mode == MTVAF_WORD_POOL_FIRST || mode == MTVAF_WORD_POOL_LAST || mode == MTVAF_WORD_POOL_MEAN;
}

}  // namespace mtvaf

using namespace mtvaf;

extern "C" {

int mtvaf_word_index(const uint8_t* attention_mask, const int* token_to_word, int* col_start, int* col_len, int* col_of_token,
                     uint8_t* word_mask, int* word_id, int* n_cols, int B, int S, int W, hipStream_t stream) {
  if (B < 1 || S < 1 || S > WP_MAX_S || W < 1) return MTVAF_ERR_SHAPE;
  if (!attention_mask || !token_to_word || !col_start || !col_len || !col_of_token || !word_mask || !word_id || !n_cols)
    return MTVAF_ERR_ARG;
  const uintptr_t ints = (uintptr_t)token_to_word | (uintptr_t)col_start | (uintptr_t)col_len | (uintptr_t)col_of_token |
                         (uintptr_t)word_id | (uintptr_t)n_cols;
  if (ints & 3) return MTVAF_ERR_ALIGN;
  hipLaunchKernelGGL(word_index_kernel, dim3(wp_grid(B)), dim3(WP_WAVES * 64), 0, stream, attention_mask, token_to_word, col_start,
                     col_len, col_of_token, word_mask, word_id, n_cols, (long)B, S, W);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

int mtvaf_word_pool_fwd(const float* x, const int* col_start, const int* col_len, float* y, int B, int S, int W, int H, int mode,
                        hipStream_t stream) {
  if (B < 1 || S < 1 || W < 1 || H < 1) return MTVAF_ERR_SHAPE;
  if (!x || !col_start || !col_len || !y || !wp_mode_ok(mode)) return MTVAF_ERR_ARG;
  const uintptr_t all = (uintptr_t)x | (uintptr_t)y;
  if ((all & 3) || (((uintptr_t)col_start | (uintptr_t)col_len) & 3)) return MTVAF_ERR_ALIGN;
  const long rows = (long)B * W;
  const dim3 grid(wp_grid(rows)), block(WP_WAVES * 64);
  if ((H & 3) == 0 && (all & 15) == 0)
    hipLaunchKernelGGL(word_pool_fwd_kernel<true>, grid, block, 0, stream, x, col_start, col_len, y, rows, S, W, H, mode);
  else
    hipLaunchKernelGGL(word_pool_fwd_kernel<false>, grid, block, 0, stream, x, col_start, col_len, y, rows, S, W, H, mode);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

int mtvaf_word_pool_bwd(const float* dy, const int* col_start, const int* col_len, const int* col_of_token, float* dx, int B, int S,
                        int W, int H, int mode, hipStream_t stream) {
  if (B < 1 || S < 1 || W < 1 || H < 1) return MTVAF_ERR_SHAPE;
  if (!dy || !col_start || !col_len || !col_of_token || !dx || !wp_mode_ok(mode)) return MTVAF_ERR_ARG;
  const uintptr_t all = (uintptr_t)dy | (uintptr_t)dx;
  if ((all & 3) || (((uintptr_t)col_start | (uintptr_t)col_len | (uintptr_t)col_of_token) & 3)) return MTVAF_ERR_ALIGN;
  const long rows = (long)B * S;
  const dim3 grid(wp_grid(rows)), block(WP_WAVES * 64);
  if ((H & 3) == 0 && (all & 15) == 0)
    hipLaunchKernelGGL(word_pool_bwd_kernel<true>, grid, block, 0, stream, dy, col_start, col_len, col_of_token, dx, rows, S, W, H, mode);
  else
    hipLaunchKernelGGL(word_pool_bwd_kernel<false>, grid, block, 0, stream, dy, col_start, col_len, col_of_token, dx, rows, S, W, H, mode);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

}  // extern "C"
