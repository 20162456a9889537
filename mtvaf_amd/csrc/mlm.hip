// Masked-LM head: token masking with compaction of the chosen rows, and cross entropy at vocabulary
// width without a [rows, V] buffer -- the logits exist one chunk [R, Vc] at a time (the library's GEMM writes it), the row
// kernels below fold a chunk into a running log-sum-exp state and, in the backward, turn a recomputed chunk into its gradient.
//
// Masking (HF DataCollatorForLanguageModeling, restated).  A token is ELIGIBLE iff its attention-mask byte is non-zero, its
// special-mask byte (if any) is zero and its id is none of the <= 8 special ids.  With three uniforms per token:
//   selected   iff eligible and u0 < probability
//   selected:  u1 < 0.8 -> mask_token_id;  else u1 < 0.9 -> min(V - 1, (int)(u2 * V));  else unchanged
// Selected tokens are numbered in row-major order; number r < capacity writes positions[r] = b * S + t and labels[r] = the
// original id and is corrupted, number r >= capacity stays as it is (counted in stats[2]).  Two launches, integers only: the first
// counts every sentence's selection (ballot + popcount per wave), the second forms the exclusive scan over the sentences in every
// block (B integer adds, any order gives the same integers), walks the sentence again with the same ballots and writes.  No
// atomics, nothing is read back.
//
// Vocabulary CE.  Per live row (row < *count and 0 <= label < V) the state is (m, s, arg, l_y): the running maximum, the running
// sum of exp(l - m), the FIRST index that attains m, the label's logit.  A chunk is reduced by one block per row in two passes
// over its (cache-resident) chunk row -- maximum with first index, then sum of exp(l - m_chunk) -- and merged into the state
// with ONE rescale of whichever side is smaller; chunks arrive in ascending order, so on a tie the earlier index stays.  Only
// differences l - m <= 0 are exponentiated: logits at +-1e4 stay finite.  The finishing block writes loss_row = m + log s - l_y,
// lse_row, and the totals (sum in double, thread t the rows t, t + 1024, ... then a fixed tree).
#include <cmath>

#include "common.h"

namespace mtvaf {

constexpr int MLM_THREADS = 256;
constexpr int MLM_WAVES = MLM_THREADS / WAVE;
constexpr int MLM_MAX_SPECIAL = 8;
constexpr int VCE_THREADS = 256;
constexpr int VCE_FINISH = 1024;
constexpr long VCE_IGNORE = -100;

struct MlmSpecial {
  int64_t id[MLM_MAX_SPECIAL];
  int n;
};

// uniforms in [0, 1) with 24 random bits each, four per Philox call; element i is a pure function of (seed, offset, i).
__global__ __launch_bounds__(256) void uniform_fill_kernel(float* __restrict__ out, long n, uint64_t seed, uint64_t offset,
                                                          const uint64_t* __restrict__ ep) {
  const uint64_t off = epoch_offset(offset, ep);
  const long n4 = (n + 3) / 4;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const uint4_ r = philox4x32((uint32_t)i, (uint32_t)((uint64_t)i >> 32), (uint32_t)off, (uint32_t)(off >> 32), (uint32_t)seed,
                                (uint32_t)(seed >> 32));
    const float u[4] = {(float)(r.x >> 8) * 0x1p-24f, (float)(r.y >> 8) * 0x1p-24f, (float)(r.z >> 8) * 0x1p-24f,
                        (float)(r.w >> 8) * 0x1p-24f};
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (4 * i + j < n) out[4 * i + j] = u[j];
  }
}

// bit 0: eligible, bit 1: selected
__device__ __forceinline__ int mlm_token_state(const int64_t* __restrict__ ids, const uint8_t* __restrict__ live,
                                               const uint8_t* __restrict__ special, const float* __restrict__ uni, long i,
                                               const MlmSpecial& sp, float probability) {
  if (!live[i] || (special && special[i])) return 0;
  const int64_t id = ids[i];
  for (int k = 0; k < sp.n; ++k)
    if (id == sp.id[k]) return 0;
  return uni[3 * i] < probability ? 3 : 1;
}

// One block per sentence: counts[b] = selected, counts[B + b] = eligible.
__global__ __launch_bounds__(MLM_THREADS) void mlm_count_kernel(const int64_t* __restrict__ ids, const uint8_t* __restrict__ live,
                                                               const uint8_t* __restrict__ special, const float* __restrict__ uni,
                                                               int* __restrict__ counts, int B, int S, MlmSpecial sp,
                                                               float probability) {
  __shared__ int wsel[MLM_WAVES], welig[MLM_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int nsel = 0, nelig = 0;  // per wave, held by every lane
  for (int t0 = 0; t0 < S; t0 += MLM_THREADS) {
    const int t = t0 + tid;
    const int st = t < S ? mlm_token_state(ids, live, special, uni, (long)b * S + t, sp, probability) : 0;
    nsel += __popcll(__ballot(st & 2));
    nelig += __popcll(__ballot(st & 1));
  }
  if (lane == 0) wsel[wave] = nsel, welig[wave] = nelig;
  __syncthreads();
  if (tid == 0) {
    int a = 0, e = 0;
    for (int w = 0; w < MLM_WAVES; ++w) a += wsel[w], e += welig[w];
    counts[b] = a;
    counts[B + b] = e;
  }
}

__global__ __launch_bounds__(MLM_THREADS) void mlm_write_kernel(const int64_t* __restrict__ ids, const uint8_t* __restrict__ live,
                                                               const uint8_t* __restrict__ special, const float* __restrict__ uni,
                                                               const int* __restrict__ counts, int64_t* __restrict__ ids_out,
                                                               int* __restrict__ positions, int64_t* __restrict__ labels,
                                                               int* __restrict__ count, int* __restrict__ stats, int B, int S,
                                                               MlmSpecial sp, float probability, long mask_token_id, int V,
                                                               int capacity) {
  __shared__ int red[2][MLM_THREADS];
  __shared__ int wcnt[MLM_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // exclusive scan over the sentences (and the totals): integer sums
  int before = 0, total = 0, elig = 0;
  for (int j = tid; j < B; j += MLM_THREADS) {
    const int c = counts[j];
    before += j < b ? c : 0;
    total += c;
    elig += counts[B + j];
  }
  red[0][tid] = before, red[1][tid] = total;
  __syncthreads();
  for (int o = MLM_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) red[0][tid] += red[0][tid + o], red[1][tid] += red[1][tid + o];
    __syncthreads();
  }
  before = red[0][0], total = red[1][0];
  __syncthreads();
  const int kept = total < capacity ? total : capacity;
  if (b == 0) {  // the eligible total, by block 0 only
    red[0][tid] = elig;
    __syncthreads();
    for (int o = MLM_THREADS / 2; o > 0; o >>= 1) {
      if (tid < o) red[0][tid] += red[0][tid + o];
      __syncthreads();
    }
    if (tid == 0) {
      *count = kept;
      stats[0] = red[0][0];
      stats[1] = total;
      stats[2] = total - kept;
    }
  }
  // the dead tail of positions / labels, shared among the blocks
  for (long r = (long)kept + (long)b * MLM_THREADS + tid; r < capacity; r += (long)gridDim.x * MLM_THREADS) {
    positions[r] = -1;
    labels[r] = VCE_IGNORE;
  }
  int base = before;  // number of the wave's first selected token of this iteration, minus the waves before it
  for (int t0 = 0; t0 < S; t0 += MLM_THREADS) {
    const int t = t0 + tid;
    const long i = (long)b * S + t;
    const int st = t < S ? mlm_token_state(ids, live, special, uni, i, sp, probability) : 0;
    const unsigned long long bal = __ballot(st & 2);
    if (lane == 0) wcnt[wave] = __popcll(bal);
    __syncthreads();
    int r = base, all = 0;
    for (int w = 0; w < MLM_WAVES; ++w) {
      r += w < wave ? wcnt[w] : 0;
      all += wcnt[w];
    }
    base += all;
    __syncthreads();
    if (t < S) {
      int64_t id = ids[i];
      if (st & 2) {
        r += __popcll(bal & ((1ull << lane) - 1ull));
        if (r < capacity) {
          positions[r] = (int)i;
          labels[r] = id;
          const float u1 = uni[3 * i + 1];
          if (u1 < 0.8f) {
            id = mask_token_id;
          } else if (u1 < 0.9f) {
            const int rnd = (int)(uni[3 * i + 2] * (float)V);
            id = rnd < V - 1 ? rnd : V - 1;
          }
        }
      }
      ids_out[i] = id;
    }
  }
}

// dsrc[map[r]][:] = d[r][:] for map[r] in [0, rows_src); dsrc was zeroed on the stream before.  The positions are distinct.
__global__ __launch_bounds__(256) void scatter_rows_kernel(const float* __restrict__ d, const int* __restrict__ map,
                                                          float* __restrict__ dsrc, int rows, int rows_src, int h4) {
  const long n = (long)rows * h4;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int r = (int)(i / h4), c = (int)(i % h4);
    const int sr = map[r];
    if (sr >= 0 && sr < rows_src) reinterpret_cast<f32x4*>(dsrc)[(long)sr * h4 + c] = reinterpret_cast<const f32x4*>(d)[i];
  }
}

// out = dy * gelu_erf'(pre): the DGELU epilogue's arithmetic (common.h) for a gradient that no product delivers -- the head's
// d(act) comes out of the LayerNorm backward.
__global__ __launch_bounds__(256) void dgelu_kernel(const float* __restrict__ dy, const float* __restrict__ pre,
                                                   float* __restrict__ out, long n4) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const f32x4 d = reinterpret_cast<const f32x4*>(dy)[i], p = reinterpret_cast<const f32x4*>(pre)[i];
    f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = d[k] * gelu_erf_grad(p[k]);
    reinterpret_cast<f32x4*>(out)[i] = o;
  }
}

// ---- vocabulary cross entropy -----------------------------------------------------------------------------------------------

__device__ __forceinline__ bool vce_live(const int64_t* __restrict__ labels, const int* __restrict__ count, int row, int V, int& y) {
  y = 0;
  if (row >= *count) return false;
  const int64_t l = labels[row];
  if (l < 0 || l >= V) return false;
  y = (int)l;
  return true;
}

// four logits of a chunk row with their bias (VEC: 16-byte loads; the host checks the alignment of rows, chunk start and width)
__device__ __forceinline__ f32x4 vce_load4(const float* __restrict__ lr, const float* __restrict__ br, int j4) {
  f32x4 l = reinterpret_cast<const f32x4*>(lr)[j4];
  if (br) l += reinterpret_cast<const f32x4*>(br)[j4];
  return l;
}

// state: m [R] | s [R] | l_y [R] | arg [R] (int32)
template <bool VEC>
__global__ __launch_bounds__(VCE_THREADS) void vocab_ce_chunk_fwd_kernel(const float* __restrict__ logits, long ld,
                                                                        const float* __restrict__ bias,
                                                                        const int64_t* __restrict__ labels,
                                                                        const int* __restrict__ count, float* __restrict__ state,
                                                                        int R, int V, int v0, int v1) {
  __shared__ float redv[VCE_THREADS / WAVE];
  __shared__ int redi[VCE_THREADS / WAVE];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int y;
  if (!vce_live(labels, count, row, V, y)) return;  // (uniform per block)
  const int Vc = v1 - v0;
  const float* __restrict__ lr = logits + (long)row * ld;
  const float* __restrict__ br = bias ? bias + v0 : nullptr;
  // pass 1: the chunk's maximum and the first index that attains it (a thread's indices rise, so '>' keeps its first)
  float mx = -INFINITY;
  int ax = 0x7fffffff;
  if (VEC) {
    for (int j4 = tid; j4 < Vc / 4; j4 += VCE_THREADS) {
      const f32x4 l = vce_load4(lr, br, j4);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (l[k] > mx) mx = l[k], ax = 4 * j4 + k;
    }
  } else {
    for (int j = tid; j < Vc; j += VCE_THREADS) {
      const float l = lr[j] + (br ? br[j] : 0.f);
      if (l > mx) mx = l, ax = j;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(mx, o, 64);
    const int oa = __shfl_xor(ax, o, 64);
    if (om > mx || (om == mx && oa < ax)) mx = om, ax = oa;
  }
  if (lane == 0) redv[wave] = mx, redi[wave] = ax;
  __syncthreads();
  mx = redv[0], ax = redi[0];
#pragma unroll
  for (int w = 1; w < VCE_THREADS / WAVE; ++w)
    if (redv[w] > mx || (redv[w] == mx && redi[w] < ax)) mx = redv[w], ax = redi[w];
  __syncthreads();
  // pass 2: sum of exp(l - mx) over the chunk, every term in (0, 1]
  float s = 0.f;
  if (VEC) {
    for (int j4 = tid; j4 < Vc / 4; j4 += VCE_THREADS) {
      const f32x4 l = vce_load4(lr, br, j4);
      s += (expf(l[0] - mx) + expf(l[1] - mx)) + (expf(l[2] - mx) + expf(l[3] - mx));
    }
  } else {
    for (int j = tid; j < Vc; j += VCE_THREADS) s += expf(lr[j] + (br ? br[j] : 0.f) - mx);
  }
  s = wave_sum(s);
  if (lane == 0) redv[wave] = s;
  __syncthreads();
  if (tid == 0) {
    s = 0.f;
    for (int w = 0; w < VCE_THREADS / WAVE; ++w) s += redv[w];
    float* sm = state + row;
    float* ss = state + R + row;
    int* sa = reinterpret_cast<int*>(state) + 3 * (long)R + row;
    if (v0 == 0) {
      *sm = mx, *ss = s, *sa = ax;
    } else {
      const float m0 = *sm, s0 = *ss;
      if (mx > m0) {
        *sm = mx, *ss = s0 * expf(m0 - mx) + s, *sa = v0 + ax;
      } else {
        *ss = s0 + s * expf(mx - m0);
      }
    }
    if (y >= v0 && y < v1) state[2 * (long)R + row] = lr[y - v0] + (br ? br[y - v0] : 0.f);
  }
}

__global__ __launch_bounds__(VCE_FINISH) void vocab_ce_finish_kernel(const float* __restrict__ state,
                                                                    const int64_t* __restrict__ labels,
                                                                    const int* __restrict__ count, float* __restrict__ loss,
                                                                    float* __restrict__ loss_row, float* __restrict__ lse_row,
                                                                    int* __restrict__ stats, int R, int V, int reduction) {
  __shared__ double red_s[VCE_FINISH];
  __shared__ int red_n[3 * VCE_FINISH];
  const int tid = threadIdx.x;
  const int cnt = *count;
  double S = 0.0;
  int live = 0, correct = 0, bad = 0;
  for (int row = tid; row < R; row += VCE_FINISH) {
    int y;
    float L = 0.f, lse = 0.f;
    if (vce_live(labels, count, row, V, y)) {
      lse = state[row] + logf(state[R + row]);
      L = lse - state[2 * (long)R + row];
      ++live;
      correct += reinterpret_cast<const int*>(state)[3 * (long)R + row] == y;
    } else if (row < cnt) {
      bad += labels[row] != VCE_IGNORE;
    }
    loss_row[row] = L;
    lse_row[row] = lse;
    S += (double)L;
  }
  red_s[tid] = S, red_n[tid] = live, red_n[VCE_FINISH + tid] = correct, red_n[2 * VCE_FINISH + tid] = bad;
  __syncthreads();
  for (int o = VCE_FINISH / 2; o > 0; o >>= 1) {
    if (tid < o) {
      red_s[tid] += red_s[tid + o];
      red_n[tid] += red_n[tid + o];
      red_n[VCE_FINISH + tid] += red_n[VCE_FINISH + tid + o];
      red_n[2 * VCE_FINISH + tid] += red_n[2 * VCE_FINISH + tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const int n = red_n[0];
    *loss = n > 0 ? (float)(reduction == 0 ? red_s[0] / (double)n : red_s[0]) : 0.f;
    stats[0] = n;
    stats[1] = red_n[VCE_FINISH];
    stats[2] = red_n[2 * VCE_FINISH];
  }
}

// In place on a recomputed chunk: dl = g_row (exp(l + bias - lse_row) - [v == label]); dead rows: zeros, nothing read.
template <bool VEC>
__global__ __launch_bounds__(VCE_THREADS) void vocab_ce_chunk_bwd_kernel(float* __restrict__ logits, long ld,
                                                                        const float* __restrict__ bias,
                                                                        const int64_t* __restrict__ labels,
                                                                        const int* __restrict__ count,
                                                                        const float* __restrict__ lse_row,
                                                                        const float* __restrict__ gout,
                                                                        const float* __restrict__ grows,
                                                                        const int* __restrict__ stats, int R, int V, int v0, int v1,
                                                                        int reduction) {
  const int row = blockIdx.x, tid = threadIdx.x;
  const int Vc = v1 - v0;
  float* __restrict__ lr = logits + (long)row * ld;
  int y;
  if (!vce_live(labels, count, row, V, y)) {
    if (VEC) {
      for (int j4 = tid; j4 < Vc / 4; j4 += VCE_THREADS) reinterpret_cast<f32x4*>(lr)[j4] = f32x4{0.f, 0.f, 0.f, 0.f};
    } else {
      for (int j = tid; j < Vc; j += VCE_THREADS) lr[j] = 0.f;
    }
    return;
  }
  float g;
  if (grows) {
    g = grows[row];
  } else {
    g = *gout;
    if (reduction == 0) g = (float)((double)g / (double)stats[0]);  // a live row exists: stats[0] >= 1
  }
  const float* __restrict__ br = bias ? bias + v0 : nullptr;
  const float lse = lse_row[row];
  const int yj = y - v0;
  if (VEC) {
    for (int j4 = tid; j4 < Vc / 4; j4 += VCE_THREADS) {
      const f32x4 l = vce_load4(lr, br, j4);
      f32x4 d;
#pragma unroll
      for (int k = 0; k < 4; ++k) d[k] = g * (expf(l[k] - lse) - (4 * j4 + k == yj ? 1.f : 0.f));
      reinterpret_cast<f32x4*>(lr)[j4] = d;
    }
  } else {
    for (int j = tid; j < Vc; j += VCE_THREADS) {
      const float p = expf(lr[j] + (br ? br[j] : 0.f) - lse);
      lr[j] = g * (p - (j == yj ? 1.f : 0.f));
    }
  }
}

}  // namespace mtvaf

using namespace mtvaf;

static bool vce_vec(const float* logits, int ld, const float* bias, int v0, int v1) {
  return ld % 4 == 0 && (v1 - v0) % 4 == 0 && v0 % 4 == 0 && !(((uintptr_t)logits) & 15) && !(((uintptr_t)bias) & 15);
}

static int vce_check(const void* logits, int ld, const void* labels, const void* count, int R, int V, int v0, int v1) {
  if (R < 1 || V < 1 || v0 < 0 || v1 <= v0 || v1 > V || ld < v1 - v0) return MTVAF_ERR_SHAPE;
  if (!logits || !labels || !count) return MTVAF_ERR_ARG;
  return MTVAF_OK;
}

extern "C" {

int mtvaf_uniform_fill(float* out, long n, uint64_t seed, uint64_t offset, hipStream_t st) {
  if (n <= 0) return MTVAF_ERR_SHAPE;
  if (!out) return MTVAF_ERR_ARG;
  const long n4 = (n + 3) / 4;
  const int blocks = (int)std::min<long>((n4 + 255) / 256, 2048);
  hipLaunchKernelGGL(uniform_fill_kernel, dim3(blocks), dim3(256), 0, st, out, n, seed, offset, rng_epoch_ptr());
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

size_t mtvaf_mlm_mask_workspace_bytes(int B) { return (size_t)2 * (B > 0 ? B : 0) * sizeof(int); }

int mtvaf_mlm_mask(const int64_t* input_ids, const uint8_t* live, const uint8_t* special_mask, const float* uniforms,
                   const int64_t* special_ids, int n_special, float probability, long mask_token_id, int vocab_size, int capacity,
                   int64_t* ids_out, int* positions, int64_t* labels, int* count, int* stats, void* workspace, size_t workspace_bytes,
                   int B, int S, hipStream_t st) {
  if (B < 1 || S < 1 || (long)B * S > 0x7fffffffL || vocab_size < 1 || capacity < 1) return MTVAF_ERR_SHAPE;
  if (!input_ids || !live || !uniforms || !ids_out || !positions || !labels || !count || !stats || n_special < 0 ||
      n_special > MLM_MAX_SPECIAL || (n_special > 0 && !special_ids) || !(probability >= 0.f && probability <= 1.f) ||
      mask_token_id < 0 || mask_token_id >= vocab_size)
    return MTVAF_ERR_ARG;
  if (!workspace || workspace_bytes < mtvaf_mlm_mask_workspace_bytes(B)) return MTVAF_ERR_WORKSPACE;
  MlmSpecial sp;
  sp.n = n_special;
  for (int k = 0; k < MLM_MAX_SPECIAL; ++k) sp.id[k] = k < n_special ? special_ids[k] : -1;  // (host array, read here)
  int* counts = static_cast<int*>(workspace);
  hipLaunchKernelGGL(mlm_count_kernel, dim3(B), dim3(MLM_THREADS), 0, st, input_ids, live, special_mask, uniforms, counts, B, S, sp,
                     probability);
  MTVAF_LAUNCH_CHECK();
  hipLaunchKernelGGL(mlm_write_kernel, dim3(B), dim3(MLM_THREADS), 0, st, input_ids, live, special_mask, uniforms, counts, ids_out,
                     positions, labels, count, stats, B, S, sp, probability, mask_token_id, vocab_size, capacity);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

int mtvaf_scatter_rows(const float* d, const int* map, float* dsrc, int rows, int rows_src, int H, hipStream_t st) {
  if (rows <= 0 || rows_src <= 0 || H <= 0 || H % 4) return MTVAF_ERR_SHAPE;
  if (!d || !map || !dsrc) return MTVAF_ERR_ARG;
  hipError_t e = hipMemsetAsync(dsrc, 0, (size_t)rows_src * H * sizeof(float), st);
  if (e != hipSuccess) return (int)e;
  const long n4 = (long)rows * (H / 4);
  const int blocks = (int)std::min<long>((n4 + 255) / 256, 4096);
  hipLaunchKernelGGL(scatter_rows_kernel, dim3(blocks), dim3(256), 0, st, d, map, dsrc, rows, rows_src, H / 4);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

int mtvaf_dgelu(const float* dy, const float* pre, float* out, long n, hipStream_t st) {
  if (n <= 0 || n % 4) return MTVAF_ERR_SHAPE;
  if (!dy || !pre || !out) return MTVAF_ERR_ARG;
  if ((((uintptr_t)dy) | ((uintptr_t)pre) | ((uintptr_t)out)) & 15) return MTVAF_ERR_ALIGN;
  const int blocks = (int)std::min<long>((n / 4 + 255) / 256, 4096);
  hipLaunchKernelGGL(dgelu_kernel, dim3(blocks), dim3(256), 0, st, dy, pre, out, n / 4);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

// the logits chunk [R, chunk] and the row state (4 words a row), each rounded to 256 bytes; no term in V
size_t mtvaf_vocab_ce_workspace_bytes(int R, int H, int V, int chunk) {
  (void)H, (void)V;
  if (R < 1 || chunk < 1) return 0;
  const size_t a = ((size_t)R * chunk * sizeof(float) + 255) / 256 * 256;
  const size_t b = ((size_t)R * 4 * sizeof(float) + 255) / 256 * 256;
  return a + b;
}

int mtvaf_vocab_ce_chunk_fwd(const float* logits, int ld, const float* bias, const int64_t* labels, const int* count, float* state,
                             int R, int V, int v0, int v1, hipStream_t st) {
  const int rc = vce_check(logits, ld, labels, count, R, V, v0, v1);
  if (rc != MTVAF_OK) return rc;
  if (!state) return MTVAF_ERR_ARG;
  if (vce_vec(logits, ld, bias, v0, v1))
    hipLaunchKernelGGL(vocab_ce_chunk_fwd_kernel<true>, dim3(R), dim3(VCE_THREADS), 0, st, logits, (long)ld, bias, labels, count, state, R,
                       V, v0, v1);
  else
    hipLaunchKernelGGL(vocab_ce_chunk_fwd_kernel<false>, dim3(R), dim3(VCE_THREADS), 0, st, logits, (long)ld, bias, labels, count, state,
                       R, V, v0, v1);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

int mtvaf_vocab_ce_finish(const float* state, const int64_t* labels, const int* count, float* loss, float* loss_row, float* lse_row,
                          int* stats, int R, int V, int reduction, hipStream_t st) {
  if (R < 1 || V < 1) return MTVAF_ERR_SHAPE;
  if (!state || !labels || !count || !loss || !loss_row || !lse_row || !stats || reduction < 0 || reduction > 1) return MTVAF_ERR_ARG;
  hipLaunchKernelGGL(vocab_ce_finish_kernel, dim3(1), dim3(VCE_FINISH), 0, st, state, labels, count, loss, loss_row, lse_row, stats, R,
                     V, reduction);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

int mtvaf_vocab_ce_chunk_bwd(float* logits, int ld, const float* bias, const int64_t* labels, const int* count, const float* lse_row,
                             const float* grad_out, const float* grad_rows, const int* stats, int R, int V, int v0, int v1,
                             int reduction, hipStream_t st) {
  const int rc = vce_check(logits, ld, labels, count, R, V, v0, v1);
  if (rc != MTVAF_OK) return rc;
  if (!lse_row || !stats || (grad_out == nullptr) == (grad_rows == nullptr) || reduction < 0 || reduction > 1) return MTVAF_ERR_ARG;
  if (vce_vec(logits, ld, bias, v0, v1))
    hipLaunchKernelGGL(vocab_ce_chunk_bwd_kernel<true>, dim3(R), dim3(VCE_THREADS), 0, st, logits, (long)ld, bias, labels, count, lse_row,
                       grad_out, grad_rows, stats, R, V, v0, v1, reduction);
  else
    hipLaunchKernelGGL(vocab_ce_chunk_bwd_kernel<false>, dim3(R), dim3(VCE_THREADS), 0, st, logits, (long)ld, bias, labels, count, lse_row,
                       grad_out, grad_rows, stats, R, V, v0, v1, reduction);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

}  // extern "C"
