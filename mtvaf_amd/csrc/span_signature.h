// Word-key signature of a token span: the keys at every change of word_index among the span's in-map tokens.  One definition,
// shared by the kernel that de-duplicates candidate spans by it (span_propose.hip) and the one that matches predicted spans
// against gold terms by it (span_score.hip).
#pragma once
#include "common.h"

namespace mtvaf {

// word-key signature equality of the spans [s1,e1] and [s2,e2]: the keys at every change of word_index among the in-map tokens
__device__ __forceinline__ bool same_signature(const int* wi, const int* wk, int s1, int e1, int s2, int e2) {
  int t1 = s1, t2 = s2, p1 = -1, p2 = -1;
  for (;;) {
    while (t1 <= e1 && (wi[t1] < 0 || wi[t1] == p1)) ++t1;
    while (t2 <= e2 && (wi[t2] < 0 || wi[t2] == p2)) ++t2;
    const bool d1 = t1 > e1, d2 = t2 > e2;
    if (d1 || d2) return d1 && d2;
    if (wk[t1] != wk[t2]) return false;
    p1 = wi[t1++];
    p2 = wi[t2++];
  }
}

}  // namespace mtvaf
