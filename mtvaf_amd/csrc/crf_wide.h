// Wide-tag CRF path (crf_wide.hip): 16 < C <= 64 tags, 1 <= S <= 512 steps.  The C ABI entry points in crf.hip dispatch
// here above crf.hip's 16-tag kernels and launch their own small epilogue kernels (batch-mean loss, parameter-gradient
// reduction) on the llh / partial arrays laid out below.
#pragma once
#include "common.h"

namespace mtvaf {

constexpr int CRF_WIDE_CMAX = 64;
constexpr int CRF_WIDE_SMAX = 512;

// what a backward kernel (either path) produces -- a template argument of the kernels:
//   CRF_GRAD_MEAN      gradients of the batch-mean NLL, upstream gradient one scalar (mtvaf_crf_nll_bwd)
//   CRF_GRAD_SENTENCE  gradients of sum_b w[b] llh[b], upstream gradient w [B] (mtvaf_crf_llh_bwd)
//   CRF_MARGINALS      the node marginals themselves: no tags, no gold counts, no edge marginals, no parameter partials
enum { CRF_GRAD_MEAN = 0, CRF_GRAD_SENTENCE = 1, CRF_MARGINALS = 2 };

// workspace, in floats, CT = C rounded up to 16:
//   alpha [B,S,CT] | sp [B,S,CT] | ui [B,S,CT] | mx [B,S] | logZ [B] | llh [B] | parameter-gradient partials [B, 2C + C*C]
struct CrfWideWs {
  float *alpha, *sp, *ui, *mx, *logz, *llh, *partial;
};
size_t crf_wide_workspace_floats(int B, int S, int C);
CrfWideWs crf_wide_ws(void* ws, int B, int S, int C);

// each launches one kernel (one wave per sentence) on `st`; crf_wide_marginals two (crf_wide_logz: the forward without the
// gold path, w.logz [B] its result; then the CRF_MARGINALS backward, which writes marg [B,S,C]).  grad: CRF_GRAD_MEAN (gout a
// scalar or NULL) or CRF_GRAD_SENTENCE (gout [B]).
int crf_wide_fwd(const float* em, const int64_t* tags, const uint8_t* mask, const float* start, const float* end,
                 const float* trans, const CrfWideWs& w, int B, int S, int C, hipStream_t st);
int crf_wide_bwd(int grad, const float* gout, const float* em, const int64_t* tags, const uint8_t* mask, const float* end,
                 const float* trans, float* dem, const CrfWideWs& w, int B, int S, int C, hipStream_t st);
int crf_wide_logz(const float* em, const uint8_t* mask, const float* start, const float* end, const float* trans,
                  const CrfWideWs& w, int B, int S, int C, hipStream_t st);
int crf_wide_marginals(const float* em, const uint8_t* mask, const float* start, const float* end, const float* trans,
                       float* marg, const CrfWideWs& w, int B, int S, int C, hipStream_t st);
int crf_wide_viterbi(const float* em, const uint8_t* mask, const float* start, const float* end, const float* trans,
                     int32_t* tags_out, int32_t* lens_out, int B, int S, int C, hipStream_t st);

}  // namespace mtvaf
