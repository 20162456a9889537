// Candidate-span proposal of the span model at eval / predict time: the eval branch of the reference's
// models/utils.py::span_annotate_candidates (:451-521) plus the host round trip around it (modules/train.py:382-410),
// as one launch with no host read-back.  Per sentence:
//   1. SI / EI = the first min(n_best, S) positions by (start / end logit descending, position ascending), taken over the
//      whole row (a masked position can use up a slot, as in the reference);
//   2. pairs (s, e) in SI x EI order, q = rank(s) * n + rank(e), kept when both tokens are in the word map, e >= s,
//      e - s + 1 <= max_len and (double)sl + (double)el >= threshold;
//   3. key = (double)sl + (double)el [- (e - s + 1) with heuristics], fp64 like the reference's Python floats;
//   4. greedy walk in (key descending, q ascending) order -- Python's stable sorted(reverse=True) -- that skips a candidate
//      whose word-key signature equals an accepted span's (nms = 1: that shares any word key with one) and stops at
//      2 * accepted >= n_best.
// One wave64 per sentence.  The walk accepts at most 16 spans, so the pairs are never sorted: every round is one wave arg-max
// over the live pairs (16 per lane, in registers) that yields the next ACCEPTED span, after which each lane drops those of its
// own pairs the new span rules out.  A pair is skipped by the reference's walk iff a span accepted before it rules it out, and
// every accepted span precedes the pairs it drops in the order, so the accepted list is the same.  No atomics; deterministic.
// Contract: finite logits; word_index rises by 0 or 1 along each run of in-map tokens.
#include "common.h"
#include "span_signature.h"  // same_signature
#include <limits.h>

namespace mtvaf {

constexpr int PROP_MAX_S = 512;   // 8 positions per lane and list
constexpr int PROP_MAX_N = 32;    // 32 * 32 pairs = 16 per lane
constexpr int PROP_LCH = PROP_MAX_S / 64;
constexpr int PROP_PCH = PROP_MAX_N * PROP_MAX_N / 64;

// n rounds of wave arg-max, lowest position on ties; idx_out[r] / val_out[r] in LDS (every lane writes the same value)
__device__ __forceinline__ void top_positions(const float (&v)[PROP_LCH], int S, int n, int lane, int* idx_out, float* val_out) {
  unsigned taken = 0;
  for (int r = 0; r < n; ++r) {
    float bv = 0.f;
    int bi = INT_MAX;
#pragma unroll
    for (int c = 0; c < PROP_LCH; ++c) {  // ascending position: a strict > keeps the lowest one
      const int s = lane + 64 * c;
      if (s < S && !(taken >> c & 1) && (bi == INT_MAX || v[c] > bv)) {
        bv = v[c];
        bi = s;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (oi != INT_MAX && (bi == INT_MAX || ov > bv || (ov == bv && oi < bi))) {
        bv = ov;
        bi = oi;
      }
    }
    bi = __shfl(bi, 0, 64);  // one answer for the wave whatever the inputs (n <= S: a position is always left)
    bv = __shfl(bv, 0, 64);
    if ((bi & 63) == lane) taken |= 1u << (bi >> 6);
    idx_out[r] = bi;
    val_out[r] = bv;
  }
}

__global__ __launch_bounds__(64) void span_propose_kernel(const float* __restrict__ logits, int ld,
                                                         const int* __restrict__ word_index, const int* __restrict__ word_key,
                                                         int64_t* __restrict__ span_starts, int64_t* __restrict__ span_ends,
                                                         int64_t* __restrict__ label_masks, float* __restrict__ span_scores,
                                                         int* __restrict__ count, int S, int n_best, int max_len,
                                                         float threshold, int use_heuristics, int nms) {
  __shared__ int wi[PROP_MAX_S], wk[PROP_MAX_S];
  __shared__ int hitpre[PROP_MAX_S + 1];  // nms: number of tokens before t whose key an accepted span holds
  __shared__ int SI[PROP_MAX_N], EI[PROP_MAX_N];
  __shared__ float SL[PROP_MAX_N], EL[PROP_MAX_N];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int n = min(n_best, S);

  float sl[PROP_LCH], el[PROP_LCH];
#pragma unroll
  for (int c = 0; c < PROP_LCH; ++c) {
    const int s = lane + 64 * c;
    sl[c] = el[c] = 0.f;
    if (s < S) {
      const float* p = logits + ((long)b * S + s) * ld;
      sl[c] = p[0];
      el[c] = p[1];
      const int w = word_index[(long)b * S + s];
      wi[s] = w;
      wk[s] = word_key ? word_key[(long)b * S + s] : w;
    }
  }
  for (int t = lane; t <= S; t += 64) hitpre[t] = 0;
  top_positions(sl, S, n, lane, SI, SL);
  top_positions(el, S, n, lane, EI, EL);
  __syncthreads();

  // the pairs of this lane: q = lane + 64 k
  double key[PROP_PCH];
  int se[PROP_PCH];  // s | e << 16
  unsigned alive = 0;
  const int n_pairs = n * n;
#pragma unroll
  for (int k = 0; k < PROP_PCH; ++k) {
    const int q = lane + 64 * k;
    key[k] = 0.0;
    se[k] = 0;
    if (q < n_pairs) {
      const int i = q / n, j = q - i * n;
      const int s = SI[i], e = EI[j];
      const double sum = (double)SL[i] + (double)EL[j];
      const int len = e - s + 1;
      if (wi[s] >= 0 && wi[e] >= 0 && e >= s && len <= max_len && sum >= (double)threshold) {
        key[k] = use_heuristics ? sum - (double)len : sum;
        se[k] = s | e << 16;
        alive |= 1u << k;
      }
    }
  }

  unsigned hit = 0;  // nms: tokens lane * 8 + c whose key an accepted span holds
  int accepted = 0;
  while (2 * accepted < n_best) {
    double bk = 0.0;
    int bq = INT_MAX;
#pragma unroll
    for (int k = 0; k < PROP_PCH; ++k)  // ascending q
      if ((alive >> k & 1) && (bq == INT_MAX || key[k] > bk)) {
        bk = key[k];
        bq = lane + 64 * k;
      }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double ok = __shfl_xor(bk, o, 64);
      const int oq = __shfl_xor(bq, o, 64);
      if (oq != INT_MAX && (bq == INT_MAX || ok > bk || (ok == bk && oq < bq))) {
        bk = ok;
        bq = oq;
      }
    }
    bq = __shfl(bq, 0, 64);
    if (bq == INT_MAX) break;  // no live pair left
    const int i = bq / n, j = bq - i * n;
    const int s = SI[i], e = EI[j];
    if (lane == 0) {
      const long o = (long)b * n_best + accepted;
      span_starts[o] = s;
      span_ends[o] = e;
      label_masks[o] = 1;
      span_scores[o] = (float)((double)SL[i] + (double)EL[j]);
    }
    if ((bq & 63) == lane) alive &= ~(1u << (bq >> 6));
    ++accepted;
    if (2 * accepted >= n_best) break;

    if (nms) {
      // a pair sharing any key with the new span goes (its own signature included: every span holds a key)
      int cnt = 0;
#pragma unroll
      for (int c = 0; c < PROP_LCH; ++c) {
        const int t = lane * PROP_LCH + c;
        if (t < S && wi[t] >= 0 && !(hit >> c & 1)) {
          const int kt = wk[t];
          for (int u = s; u <= e; ++u)
            if (wi[u] >= 0 && wk[u] == kt) {
              hit |= 1u << c;
              break;
            }
        }
        cnt += hit >> c & 1;
      }
      int inc = cnt;  // inclusive scan over the lanes
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(inc, o, 64);
        if (lane >= o) inc += v;
      }
      int run = inc - cnt;
      __syncthreads();  // reads of the previous round's hitpre are done
#pragma unroll
      for (int c = 0; c < PROP_LCH; ++c) {
        const int t = lane * PROP_LCH + c;
        run += hit >> c & 1;
        if (t < S) hitpre[t + 1] = run;
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < PROP_PCH; ++k)
        if (alive >> k & 1) {
          const int cs = se[k] & 0xffff, ce = se[k] >> 16;
          if (hitpre[ce + 1] - hitpre[cs] > 0) alive &= ~(1u << k);
        }
    } else {
#pragma unroll
      for (int k = 0; k < PROP_PCH; ++k)
        if (alive >> k & 1) {
          const int cs = se[k] & 0xffff, ce = se[k] >> 16;
          if (same_signature(wi, wk, s, e, cs, ce)) alive &= ~(1u << k);
        }
    }
  }

  // padding, as the reference pads: zeros
  for (int r = accepted + lane; r < n_best; r += 64) {
    const long o = (long)b * n_best + r;
    span_starts[o] = 0;
    span_ends[o] = 0;
    label_masks[o] = 0;
    span_scores[o] = 0.f;
  }
  if (lane == 0) count[b] = accepted;
}

}  // namespace mtvaf

using namespace mtvaf;

extern "C" {

int mtvaf_span_propose(const float* logits, int ld, const int* word_index, const int* word_key, int64_t* span_starts,
                       int64_t* span_ends, int64_t* label_masks, float* span_scores, int* count, int B, int S, int n_best,
                       int max_len, float threshold, int use_heuristics, int nms, hipStream_t st) {
  if (B <= 0 || S < 1 || S > PROP_MAX_S || n_best < 1 || n_best > PROP_MAX_N || ld < 2) return MTVAF_ERR_SHAPE;
  if (nms != 0 && nms != 1) return MTVAF_ERR_ARG;
  hipLaunchKernelGGL(span_propose_kernel, dim3(B), dim3(64), 0, st, logits, ld, word_index, word_key, span_starts, span_ends,
                     label_masks, span_scores, count, S, n_best, max_len, threshold, use_heuristics, nms);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

}  // extern "C"
