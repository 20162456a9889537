// N-best Viterbi of the linear-chain CRF head: the K best tag sequences of every sentence with their unnormalised scores,
// their log-probabilities (score - logZ, logZ from the forward recursion of crf.hip / crf_wide.hip) and the number of
// sequences that exist.  pytorch-crf's decode(nbest=...) on the device; 1 <= K <= 8, 1 <= C <= 64, 1 <= S <= 512.
//
// One wave64 per sentence, tag j on lane j.  best[t][j][0..K-1], the K best scores of a prefix that ends in tag j at step
// t in non-increasing order, is K registers of lane j; rank r of tag i is read across lanes with v_readlane (i is
// wave-uniform, r a constant of the unrolled code), so the score panels never pass through memory.  A step offers lane j
// the candidates best[t-1][i][r] + trans[i][j] in the order i = 0 .. C-1, r = 0 .. K-1 and keeps a sorted top-K by insertion;
// a candidate enters only if it is STRICTLY greater than the current K-th, and moves up only past strictly smaller ones:
//   * ties fall to the lower previous tag, then the lower previous rank (rank 0 is mtvaf_crf_viterbi's "first maximum");
//   * list i is sorted, so the first refusal ends it: a step costs C refusals plus the insertions, not C * K offers;
//   * a missing rank is -inf, -inf + x is never greater than anything, so it never extends.
// The column trans[.][j] comes from the LDS (row stride 65: lanes hit distinct banks), emissions are fetched one step ahead.
// Back-pointers (previous tag << 3 | previous rank, 16 bits) are K * C * S per sentence -- 512 KiB at the limits -- and live in
// the caller's workspace as [b][t][rank][tag]; the backtrace stages them through the LDS in runs of whole steps with coalesced
// loads and walks the K paths on K lanes.  The mask is a prefix mask: the length is the count of leading ones, steps behind it
// are not run, end[] is added at step len-1.
// The n-best kernel sets no function attribute (33 KB of static LDS).  With logprob_out the call also runs crf_logz (crf.h), which
// for C <= 16 and S above about 470 opts into more than 64 KB of LDS at the call: stream capture of that shape is as safe as
// capture of mtvaf_crf_marginals, and a first call outside the capture settles it.
#include "crf.h"
#include "crf_chain.h"

namespace mtvaf {

constexpr int NB_MAX_K = 8;
constexpr int NB_MAX_C = CRF_CHAIN_CMAX;
constexpr int NB_LD = CRF_CHAIN_LD;   // row stride of trans in the LDS
constexpr int NB_STAGE = 8192;        // back-pointers per LDS stage: at least 16 steps at K = 8, C = 64

// v enters the sorted list at the bottom and rises past strictly smaller entries (v > top[K-1] is the caller's test)
template <int K>
__device__ __forceinline__ void nb_insert(float (&top)[K], int (&id)[K], float v, int code) {
  top[K - 1] = v;
  id[K - 1] = code;
#pragma unroll
  for (int q = K - 1; q > 0; --q) {
    const bool up = top[q] > top[q - 1];
    const float hi = up ? top[q] : top[q - 1], lo = up ? top[q - 1] : top[q];
    const int ihi = up ? id[q] : id[q - 1], ilo = up ? id[q - 1] : id[q];
    top[q - 1] = hi;
    top[q] = lo;
    id[q - 1] = ihi;
    id[q] = ilo;
  }
}

// offer the sorted list of tag i (sc[r] on lane i) plus w to this lane's top-K
template <int K>
__device__ __forceinline__ void nb_offer(float (&top)[K], int (&id)[K], const float (&sc)[K], int i, float w) {
#pragma unroll
  for (int r = 0; r < K; ++r) {
    const float v = lane_val(sc[r], i) + w;
    if (!(v > top[K - 1])) break;
    nb_insert<K>(top, id, v, i * NB_MAX_K + r);
  }
}

template <int K>
__global__ __launch_bounds__(64) void crf_nbest_kernel(const float* __restrict__ em, const uint8_t* __restrict__ mask,
                                                      const float* __restrict__ start, const float* __restrict__ end,
                                                      const float* __restrict__ trans, uint16_t* __restrict__ bp,
                                                      const float* __restrict__ logz, int32_t* __restrict__ tags_out,
                                                      float* __restrict__ scores_out, float* __restrict__ logprob_out,
                                                      int32_t* __restrict__ n_paths_out, int S, int C) {
  __shared__ float s_trans[NB_MAX_C * NB_LD];
  __shared__ uint16_t s_bp[NB_STAGE];
  const int b = blockIdx.x, lane = threadIdx.x;
  stage_trans(s_trans, trans, C, lane, 64);
  int len = S;  // leading ones of the mask
  for (int w = 0; w < S; w += 64) {
    const int c = w + lane;
    const uint64_t z = __ballot(c < S && mask[(long)b * S + c] == 0);
    if (z && len == S) len = w + __ffsll((long long)z) - 1;
  }
  len = max(len, 1);  // (mask[:,0] == 1 is the caller's side of the contract: no index below depends on it)
  __syncthreads();

  const bool act = lane < C;
  const int j = act ? lane : C - 1;  // lanes >= C shadow the last tag: never read by lane_val, nothing stored
  const float* e = em + (long)b * S * C + j;
  float sc[K];
  sc[0] = act ? start[j] + e[0] : -INFINITY;
#pragma unroll
  for (int r = 1; r < K; ++r) sc[r] = -INFINITY;
  uint16_t* bpw = bp + (size_t)b * S * K * C + j;
  float en = len > 1 ? e[C] : 0.f;
  for (int t = 1; t < len; ++t) {
    const float et = en;
    if (t + 1 < len) en = e[(long)(t + 1) * C];
    float top[K];
    int id[K];
#pragma unroll
    for (int r = 0; r < K; ++r) {
      top[r] = -INFINITY;
      id[r] = 0;  // (a rank that stays -inf points at tag 0, rank 0: in bounds, never on a returned path)
    }
    const float* tc = s_trans + j;
    int i = 0;
    for (; i + 4 <= C; i += 4) {
      const float w0 = tc[i * NB_LD], w1 = tc[(i + 1) * NB_LD], w2 = tc[(i + 2) * NB_LD], w3 = tc[(i + 3) * NB_LD];
      nb_offer<K>(top, id, sc, i, w0);
      nb_offer<K>(top, id, sc, i + 1, w1);
      nb_offer<K>(top, id, sc, i + 2, w2);
      nb_offer<K>(top, id, sc, i + 3, w3);
    }
    for (; i < C; ++i) nb_offer<K>(top, id, sc, i, tc[i * NB_LD]);
#pragma unroll
    for (int r = 0; r < K; ++r) {
      sc[r] = act ? top[r] + et : -INFINITY;
      if (act) bpw[((size_t)t * K + r) * C] = (uint16_t)id[r];
    }
  }

  // the K best of best[len-1][i][r] + end[i], lower last tag first, then lower rank: the same on every lane
  float top[K];
  int id[K];
#pragma unroll
  for (int r = 0; r < K; ++r) {
    top[r] = -INFINITY;
    id[r] = 0;
  }
  for (int i = 0; i < C; ++i) nb_offer<K>(top, id, sc, i, end[i]);
  int n_paths = 1;  // min(K, C^len)
  for (int t = 0; t < len && n_paths < K; ++t) n_paths = min(n_paths * C, K);
  float my = -INFINITY;
  int code = 0;
#pragma unroll
  for (int r = 0; r < K; ++r)
    if (lane == r) {
      my = top[r];
      code = id[r];
    }
  const bool walker = lane < n_paths;  // lane k walks path k
  int32_t* out = tags_out + ((size_t)b * K + lane) * S;
  int tag = code >> 3, rank = code & 7;
  if (walker) out[len - 1] = tag;
  __syncthreads();  // this wave's back-pointer stores are visible to its loads
  const int per = K * C, steps = NB_STAGE / per;
  const uint16_t* bpr = bp + (size_t)b * S * per;
  for (int hi = len - 1; hi >= 1; hi -= steps) {  // steps lo .. hi in the LDS
    const int lo = max(1, hi - steps + 1), n = (hi - lo + 1) * per;
    const uint16_t* src = bpr + (size_t)lo * per;
    for (int x = lane; x < n; x += 64) s_bp[x] = src[x];
    __syncthreads();
    if (walker)
      for (int t = hi; t >= lo; --t) {
        const int c = s_bp[((t - lo) * K + rank) * C + tag];
        tag = c >> 3;
        rank = c & 7;
        out[t - 1] = tag;
      }
    __syncthreads();  // the next run overwrites the stage
  }
  int32_t* fill = tags_out + (size_t)b * K * S;
  for (int x = lane; x < K * S; x += 64)
    if (x / S >= n_paths || x % S >= len) fill[x] = -1;
  if (lane < K) {
    const float s = walker ? my : -INFINITY;
    scores_out[(size_t)b * K + lane] = s;
    if (logprob_out) logprob_out[(size_t)b * K + lane] = walker ? s - logz[b] : -INFINITY;
  }
  if (lane == 0) n_paths_out[b] = n_paths;
}

}  // namespace mtvaf

using namespace mtvaf;

namespace {
bool nb_bad_shape(int B, int S, int C, int K) {
  return bad_shape(B, S, C) || K < 1 || K > NB_MAX_K;
}
// workspace: back-pointers u16 [B,S,K,C] (rounded up to 256 bytes) | logZ f32 [B] (rounded up to 256 bytes) | the forward
// recursion's own workspace (mtvaf_crf_workspace_bytes)
size_t nb_round(size_t n) { return (n + 255) & ~(size_t)255; }
size_t nb_bp_bytes(int B, int S, int C, int K) { return nb_round((size_t)B * S * K * C * sizeof(uint16_t)); }
size_t nb_logz_bytes(int B) { return nb_round((size_t)B * sizeof(float)); }
}  // namespace

extern "C" {

size_t mtvaf_crf_nbest_workspace_bytes(int B, int S, int C, int K) {
  if (nb_bad_shape(B, S, C, K)) return 0;
  return nb_bp_bytes(B, S, C, K) + nb_logz_bytes(B) + mtvaf_crf_workspace_bytes(B, S, C);
}

int mtvaf_crf_nbest(const float* emissions, const uint8_t* mask, const float* start, const float* end, const float* trans,
                    int K, int32_t* tags_out, float* scores_out, float* logprob_out, int32_t* n_paths_out, int B, int S,
                    int C, void* workspace, size_t workspace_bytes, hipStream_t st) {
  if (nb_bad_shape(B, S, C, K)) return MTVAF_ERR_SHAPE;
  if (workspace_bytes < mtvaf_crf_nbest_workspace_bytes(B, S, C, K)) return MTVAF_ERR_WORKSPACE;
  uint16_t* bp = (uint16_t*)workspace;
  float* logz = (float*)((char*)workspace + nb_bp_bytes(B, S, C, K));
  if (logprob_out) {
    void* fwd_ws = (char*)logz + nb_logz_bytes(B);
    if (int rc = crf_logz(emissions, mask, start, end, trans, logz, B, S, C, fwd_ws, st)) return rc;
  }
#define NB_LAUNCH(KK)                                                                                                  \
  case KK:                                                                                                             \
    hipLaunchKernelGGL(crf_nbest_kernel<KK>, dim3(B), dim3(64), 0, st, emissions, mask, start, end, trans, bp, logz,   \
                       tags_out, scores_out, logprob_out, n_paths_out, S, C);                                          \
    break;
  switch (K) {
    NB_LAUNCH(1) NB_LAUNCH(2) NB_LAUNCH(3) NB_LAUNCH(4) NB_LAUNCH(5) NB_LAUNCH(6) NB_LAUNCH(7) NB_LAUNCH(8)
  }
#undef NB_LAUNCH
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

}  // extern "C"
