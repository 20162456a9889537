// Host-side entry points of crf.hip that other translation units of the CRF head call (crf_nbest.hip).
#pragma once
#include "common.h"

namespace mtvaf {

// Both paths (C <= 16 and the wide one): logz[b] = log-partition of sentence b by the forward recursion without the gold path -- the
// first launch of mtvaf_crf_marginals.  `workspace` holds mtvaf_crf_workspace_bytes(B, S, C) and is overwritten; the shape is the
// caller's check.  For C <= 16 and S above about 470 the recursion needs more than 64 KB of LDS and opts in with
// hipFuncSetAttribute at the call, as under mtvaf_crf_marginals.
int crf_logz(const float* em, const uint8_t* mask, const float* start, const float* end, const float* trans, float* logz,
             int B, int S, int C, void* workspace, hipStream_t st);

// Where crf_logz (and every other forward launch on `workspace`) leaves the alphas: row t of sentence b starts at
// result + ((size_t)b * S + t) * *ld and holds C floats, alpha_t[.] divided by a positive constant of that row (the scaled
// linear domain of both paths); rows of masked columns repeat the last unmasked one.
const float* crf_alpha(const void* workspace, int B, int S, int C, int* ld);

}  // namespace mtvaf
