// Aspect-level scoring of the span model's predictions on the device: the counting of modules/eval_metrics.py::eval_absa
// (:80-124) that the reference trainer reaches through per-sentence host copies (modules/train.py:200-209).  One launch ADDS,
// per polarity class, the retrieved, relevant and common terms of a batch into a 64-bit device counter.
//
// The rule is exact on integers apart from one arg-max over fp32.  Per sentence:
//   valid        a span (s, e) with 0 <= s <= e < S and both end tokens in the word map (word_index >= 0);
//   signature    word_key[t] wherever word_index[t] differs from the previous in-map token of the span (span_signature.h: the
//                definition mtvaf_span_propose de-duplicates by);
//   predicted    slot n exists iff label_masks != 0; its class is the lowest k whose logit no other exceeds; it adds 1 to
//                retrieved[class], valid or not;
//   gold         slot g exists iff gold_masks != 0; it adds 1 to relevant[gold_class], or to relevant_other with a class outside
//                [0, K); an invalid one (a term the feature truncated) is counted and can never be matched;
//   hit          a valid predicted slot with some valid gold slot of equal signature and equal class: 1 to common[class], however
//                many gold slots match; matched_gold is the lowest of them.
// One wave64 per sentence, four sentences per block.  The sentence's word_index / word_key are staged in the LDS; lanes 0..31
// read one predicted slot each, lanes 32..63 one gold slot each, and park (span, class) in the LDS; the N * G <= 1024 pairs are
// spread over the lanes, a match lowers the slot's entry with an LDS integer min.  Counts are wave ballots, summed per block in
// LDS integers, and leave as one 64-bit global atomic per block and non-zero counter: integer sums commute, so the counter is
// bit-reproducible.  No floating-point arithmetic after the arg-max.
#include "common.h"
#include "span_signature.h"
#include <limits.h>

namespace mtvaf {

constexpr int SC_MAX_S = 512;
constexpr int SC_MAX_N = 32;  // predicted slots: lanes 0..31
constexpr int SC_MAX_G = 32;  // gold slots: lanes 32..63
constexpr int SC_MAX_K = 8;
constexpr int SC_WAVES = 4;   // sentences in flight per block
constexpr int SC_MAX_CNT = 3 * SC_MAX_K + 2;

__global__ __launch_bounds__(64 * SC_WAVES) void span_counts_kernel(
    const int64_t* __restrict__ span_starts, const int64_t* __restrict__ span_ends, const int64_t* __restrict__ label_masks,
    const float* __restrict__ logits, const int64_t* __restrict__ gold_starts, const int64_t* __restrict__ gold_ends,
    const int64_t* __restrict__ gold_class, const int64_t* __restrict__ gold_masks, const int* __restrict__ word_index,
    const int* __restrict__ word_key, int B, int S, int N, int G, int K, unsigned long long* __restrict__ counts,
    int* __restrict__ pred_class, int* __restrict__ matched_gold) {
  __shared__ int s_wi[SC_WAVES][SC_MAX_S], s_wk[SC_WAVES][SC_MAX_S];
  __shared__ int s_span[SC_WAVES][64];  // per lane's slot: s | e << 16, -1 when it cannot match (absent or invalid)
  __shared__ int s_cls[SC_WAVES][64];   // class of the slot: 0..K-1, K = a gold class outside the range, -1 = absent
  __shared__ int s_match[SC_WAVES][SC_MAX_N];
  __shared__ unsigned s_cnt[SC_MAX_CNT];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n_cnt = 3 * K + 2;
  for (int i = tid; i < n_cnt; i += 64 * SC_WAVES) s_cnt[i] = 0;

  int* wi = s_wi[wave];
  int* wk = s_wk[wave];
  const bool gold_side = lane >= 32;
  const int slot = lane & 31;
  const bool in_range = slot < (gold_side ? G : N);

  // every wave of the block makes the same number of trips: the barriers below are block-wide
  for (int base = blockIdx.x * SC_WAVES; base < B; base += gridDim.x * SC_WAVES) {
    const int row = base + wave;
    const bool active = row < B;  // wave-uniform
    if (active) {
      for (int t = lane; t < S; t += 64) {
        const int w = word_index[(long)row * S + t];
        wi[t] = w;
        wk[t] = word_key ? word_key[(long)row * S + t] : w;
      }
      if (lane < SC_MAX_N) s_match[wave][lane] = INT_MAX;
    }
    __syncthreads();  // the word map is in the LDS (and, on the first trip, the block's counters are zero)

    int cls = -1;
    const long o = (long)row * (gold_side ? G : N) + slot;
    if (active) {
      int span = -1;
      if (in_range && (gold_side ? gold_masks : label_masks)[o] != 0) {
        if (gold_side) {
          const int64_t c = gold_class[o];
          cls = c >= 0 && c < K ? (int)c : K;
        } else {
          const float* l = logits + o * K;
          float best = l[0];
          cls = 0;
          for (int k = 1; k < K; ++k) {  // ascending k: a strict > keeps the lowest one
            const float v = l[k];
            if (v > best) {
              best = v;
              cls = k;
            }
          }
        }
        const int64_t s = (gold_side ? gold_starts : span_starts)[o], e = (gold_side ? gold_ends : span_ends)[o];
        if (s >= 0 && s <= e && e < S && wi[s] >= 0 && wi[e] >= 0) span = (int)s | (int)e << 16;
      }
      s_span[wave][lane] = span;
      s_cls[wave][lane] = cls;
    }
    __syncthreads();  // the slots are in the LDS

    if (active) {
      const int pairs = N * G;
      for (int p = lane; p < pairs; p += 64) {
        const int n = p / G, g = p - n * G;
        const int sp = s_span[wave][n], sg = s_span[wave][32 + g];
        if (sp >= 0 && sg >= 0 && s_cls[wave][n] == s_cls[wave][32 + g] &&
            same_signature(wi, wk, sp & 0xffff, sp >> 16, sg & 0xffff, sg >> 16))
          atomicMin(&s_match[wave][n], g);
      }
    }
    __syncthreads();  // every pair has been looked at

    if (active) {
      const bool pred_slot = !gold_side && in_range;
      const int mg = pred_slot ? s_match[wave][slot] : INT_MAX;
      const bool hit = mg != INT_MAX;
      if (pred_slot) {
        if (pred_class) pred_class[o] = cls;
        if (matched_gold) matched_gold[o] = hit ? mg : -1;
      }
      unsigned mine[3] = {0, 0, 0};  // lane k < K: retrieved, relevant, common of class k
      for (int k = 0; k < K; ++k) {
        const unsigned ret = __popcll(__ballot(!gold_side && cls == k));
        const unsigned rel = __popcll(__ballot(gold_side && cls == k));
        const unsigned com = __popcll(__ballot(hit && cls == k));
        if (lane == k) {
          mine[0] = ret;
          mine[1] = rel;
          mine[2] = com;
        }
      }
      const unsigned other = __popcll(__ballot(gold_side && cls == K));
      if (lane < K) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
          if (mine[j]) atomicAdd(&s_cnt[3 * lane + j], mine[j]);
      } else if (lane == K) {
        if (other) atomicAdd(&s_cnt[3 * K], other);
        atomicAdd(&s_cnt[3 * K + 1], 1u);
      }
    }
    __syncthreads();  // the next sentence overwrites the word map and the slots
  }

  for (int i = tid; i < n_cnt; i += 64 * SC_WAVES) {
    const unsigned v = s_cnt[i];
    if (v) atomicAdd(&counts[i], (unsigned long long)v);
  }
}

}  // namespace mtvaf

using namespace mtvaf;

extern "C" {

int mtvaf_span_counts(const int64_t* span_starts, const int64_t* span_ends, const int64_t* label_masks, const float* logits,
                      const int64_t* gold_starts, const int64_t* gold_ends, const int64_t* gold_class,
                      const int64_t* gold_masks, const int* word_index, const int* word_key, int B, int S, int N, int G, int K,
                      int64_t* counts, int* pred_class, int* matched_gold, hipStream_t st) {
  if (B <= 0 || S < 1 || S > SC_MAX_S || N < 1 || N > SC_MAX_N || G < 1 || G > SC_MAX_G || K < 2 || K > SC_MAX_K)
    return MTVAF_ERR_SHAPE;
  if ((long)B * SC_MAX_N > 0x7fffffffL) return MTVAF_ERR_SHAPE;  // a block's LDS counters are 32-bit
  const int blocks = min((B + SC_WAVES - 1) / SC_WAVES, 1024);
  hipLaunchKernelGGL(span_counts_kernel, dim3(blocks), dim3(64 * SC_WAVES), 0, st, span_starts, span_ends, label_masks, logits,
                     gold_starts, gold_ends, gold_class, gold_masks, word_index, word_key, B, S, N, G, K,
                     (unsigned long long*)counts, pred_class, matched_gold);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

}  // extern "C"
