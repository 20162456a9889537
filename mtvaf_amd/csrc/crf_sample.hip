// Forward-filter backward-sample of the linear-chain CRF head: K tag sequences of every sentence drawn from the posterior
// p(y | x), with their unnormalised scores and log-probabilities.  1 <= K <= 64, 1 <= C <= 64, 1 <= S <= 512.
//
// The forward pass is the one of mtvaf_crf_marginals (crf_logz of crf.hip / crf_wide.hip): it leaves logZ and, in its
// workspace, a scaled alpha of every column, a_t[i] = alpha_t[i] / K_t.  A draw only needs alpha_t up to a constant of the
// column -- the weights below are normalised by their own maximum -- so log a_t[i] stands in for the log-alpha and no third
// recursion is written.
//
// Draw of sample k of sentence b (length L = the leading ones of the prefix mask), columns t = L-1 .. 0:
//     x_i = log a_t[i] + (t == L-1 ? end[i] : trans[i][y_{t+1}]),   w_i = exp(x_i - max_i x_i),   F_j = sum_{i <= j} w_i
// in ascending tag order in fp32; the tag is the smallest j with F_j > u * F_{C-1}, u the uniform of (b, k, t); if rounding
// leaves no such j, the highest j with w_j > 0.
//
// One wave64 per sentence, sample k on lane k: the K chains walk the same alphas independently, so a lane sums the C
// weights serially and no wave-wide scan is needed; K = 64 costs what K = 1 costs.  Columns are staged through the LDS in
// runs of 32: log a_t[i] (read as a broadcast: every lane the same address), the emissions (gathered by tag for the score),
// the uniforms (row stride 33: conflict-free).  trans is a [C][65] image in the LDS, gathered as trans[i][y] with i uniform
// -- lanes with equal y broadcast, lanes of one half-wave that differ by 32 in y share a bank (2-way at worst).  A lane parks
// its weights in a private LDS column (s_w[i][lane]: conflict-free) between the summing and the searching pass.
//
// Uniforms: handed in ([B,K,S] fp32, the test mode), or Philox4x32-10 (common.h) with
//     counter = (lo32(idx), hi32(idx), lo32(offset), hi32(offset)),  idx = (b * 64 + k) * 128 + (t >> 2),  key = (lo32(seed), hi32(seed)),
// word t & 3 of the four results, u = (word >> 8) * 2^-24 in [0, 1).  offset passes through epoch_offset (common.h) like a dropout
// site's, so a captured launch draws fresh samples on every replay once the epoch word is advanced.
#include "crf.h"
#include "crf_chain.h"

namespace mtvaf {

constexpr int SM_MAX_K = 64;
constexpr int SM_MAX_C = CRF_CHAIN_CMAX;
constexpr int SM_LD = CRF_CHAIN_LD;  // row stride of trans in the LDS
constexpr int SM_T = 32;             // columns per LDS stage
constexpr int SM_ULD = SM_T + 1;     // row stride of the staged uniforms

__device__ __forceinline__ float sm_uniform(uint64_t seed, uint64_t offset, int b, int k, int t) {
  const uint64_t idx = ((uint64_t)b * 64 + (uint64_t)k) * 128 + (uint64_t)(t >> 2);
  const uint4_ r = philox4x32((uint32_t)idx, (uint32_t)(idx >> 32), (uint32_t)offset, (uint32_t)(offset >> 32), (uint32_t)seed,
                              (uint32_t)(seed >> 32));
  const int q = t & 3;
  const uint32_t word = q == 0 ? r.x : (q == 1 ? r.y : (q == 2 ? r.z : r.w));
  return (float)(word >> 8) * 5.9604644775390625e-08f;  // 2^-24: exact
}

__global__ __launch_bounds__(64) void crf_sample_kernel(const float* __restrict__ em, const uint8_t* __restrict__ mask,
                                                       const float* __restrict__ start, const float* __restrict__ end,
                                                       const float* __restrict__ trans, const float* __restrict__ alpha,
                                                       int lda, const float* __restrict__ logz, int K,
                                                       const float* __restrict__ uniforms, uint64_t seed, uint64_t offset,
                                                       const uint64_t* __restrict__ epoch, int32_t* __restrict__ tags_out,
                                                       float* __restrict__ scores_out, float* __restrict__ logprob_out,
                                                       float* __restrict__ uniforms_out, int S, int C) {
  __shared__ float s_trans[SM_MAX_C * SM_LD];
  __shared__ float s_start[SM_MAX_C], s_end[SM_MAX_C];
  __shared__ float s_la[SM_T * 64];           // log a_t[i] of the staged columns, -inf for i >= C
  __shared__ float s_em[SM_T * 64];           // their emissions
  __shared__ float s_u[SM_MAX_K * SM_ULD];    // their uniforms, [k][column]
  __shared__ float s_w[SM_MAX_C * 64];        // [i][lane]: the weights of the column a lane is drawing
  const int b = blockIdx.x, lane = threadIdx.x;
  stage_trans(s_trans, trans, C, lane, 64);
  if (lane < C) {
    s_start[lane] = start[lane];
    s_end[lane] = end[lane];
  }
  int len = S;  // leading ones of the mask
  for (int w = 0; w < S; w += 64) {
    const int c = w + lane;
    const uint64_t z = __ballot(c < S && mask[(long)b * S + c] == 0);
    if (z && len == S) len = w + __ffsll((long long)z) - 1;
  }
  len = max(len, 1);  // (mask[:,0] == 1 is the caller's side of the contract: no index below depends on it)
  if (!uniforms) offset = epoch_offset(offset, epoch);

  const bool walker = lane < K;          // lane k draws sample k; the others shadow sample K-1 and store nothing
  const int ku = walker ? lane : K - 1;
  const size_t row = (size_t)b * K + ku;
  int32_t* out = tags_out + row * S;
  int y = 0;
  float sc = 0.f;
  for (int hi = len - 1; hi >= 0; hi -= SM_T) {  // columns lo .. hi in the LDS
    const int lo = max(0, hi - SM_T + 1), n = hi - lo + 1;
    __syncthreads();  // the previous run has been walked (first trip: trans, start and end are in the LDS)
    for (int tt = 0; tt < n; ++tt) {
      const size_t r = (size_t)b * S + lo + tt;
      s_la[tt * 64 + lane] = lane < C ? logf(alpha[r * lda + lane]) : -INFINITY;
      s_em[tt * 64 + lane] = lane < C ? em[r * C + lane] : 0.f;
    }
    for (int x = lane; x < K * n; x += 64) {
      const int k = x / n, tt = x - k * n, t = lo + tt;
      const size_t at = ((size_t)b * K + k) * S + t;
      const float u = uniforms ? uniforms[at] : sm_uniform(seed, offset, b, k, t);
      s_u[k * SM_ULD + tt] = u;
      if (uniforms_out) uniforms_out[at] = u;
    }
    __syncthreads();
    for (int t = hi; t >= lo; --t) {
      const int tt = t - lo;
      const float* la = s_la + tt * 64;
      const bool last = t == len - 1;
      const float* add = last ? s_end : s_trans + y;  // x_i = la[i] + add[i * step]
      const int step = last ? 1 : SM_LD;
      float m = -INFINITY;
      for (int i = 0; i < C; ++i) m = fmaxf(m, la[i] + add[i * step]);
      if (!(m > -INFINITY)) m = 0.f;  // no finite x: every weight is 0 and the fallback below takes tag 0
      float total = 0.f;
      int top = 0;  // the highest tag with a positive weight
      for (int i = 0; i < C; ++i) {
        const float w = __expf((la[i] + add[i * step]) - m);
        s_w[i * 64 + lane] = w;
        total += w;
        if (w > 0.f) top = i;
      }
      const float thr = s_u[ku * SM_ULD + tt] * total;
      float run = 0.f;
      int tag = -1;
      for (int i = 0; i < C; ++i) {
        run += s_w[i * 64 + lane];  // the same additions in the same order as `total`
        if (tag < 0 && run > thr) tag = i;
      }
      if (tag < 0) tag = top;
      sc += last ? s_end[tag] + s_em[tt * 64 + tag] : s_trans[tag * SM_LD + y] + s_em[tt * 64 + tag];
      if (walker) out[t] = tag;
      y = tag;
    }
  }
  sc += s_start[y];
  if (walker) {
    scores_out[row] = sc;
    if (logprob_out) logprob_out[row] = sc - logz[b];
  }
  for (int x = lane; x < K * S; x += 64)
    if (x % S >= len) {
      tags_out[(size_t)b * K * S + x] = -1;
      if (uniforms_out) uniforms_out[(size_t)b * K * S + x] = 0.f;
    }
}

}  // namespace mtvaf

using namespace mtvaf;

namespace {
bool sm_bad_shape(int B, int S, int C, int K) {
  return bad_shape(B, S, C) || K < 1 || K > SM_MAX_K;
}
// workspace: logZ f32 [B] (rounded up to 256 bytes) | the forward recursion's own workspace (mtvaf_crf_workspace_bytes), whose
// alpha rows the kernel reads
size_t sm_logz_bytes(int B) { return ((size_t)B * sizeof(float) + 255) & ~(size_t)255; }
}  // namespace

extern "C" {

size_t mtvaf_crf_sample_workspace_bytes(int B, int S, int C, int K) {
  if (sm_bad_shape(B, S, C, K)) return 0;
  return sm_logz_bytes(B) + mtvaf_crf_workspace_bytes(B, S, C);
}

int mtvaf_crf_sample(const float* emissions, const uint8_t* mask, const float* start, const float* end, const float* trans,
                     int K, const float* uniforms, uint64_t seed, uint64_t offset, int32_t* tags_out, float* scores_out,
                     float* logprob_out, float* uniforms_out, int B, int S, int C, void* workspace, size_t workspace_bytes,
                     hipStream_t st) {
  if (sm_bad_shape(B, S, C, K)) return MTVAF_ERR_SHAPE;
  if (workspace_bytes < mtvaf_crf_sample_workspace_bytes(B, S, C, K)) return MTVAF_ERR_WORKSPACE;
  float* logz = (float*)workspace;
  void* fwd_ws = (char*)workspace + sm_logz_bytes(B);
  if (int rc = crf_logz(emissions, mask, start, end, trans, logz, B, S, C, fwd_ws, st)) return rc;
  int lda = 0;
  const float* alpha = crf_alpha(fwd_ws, B, S, C, &lda);
  hipLaunchKernelGGL(crf_sample_kernel, dim3(B), dim3(64), 0, st, emissions, mask, start, end, trans, alpha, lda, logz, K,
                     uniforms, seed, offset, rng_epoch_ptr(), tags_out, scores_out, logprob_out, uniforms_out, S, C);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

}  // extern "C"
