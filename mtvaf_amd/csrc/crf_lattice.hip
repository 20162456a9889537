// Linear-chain CRF over a per-position TAG SET ("lattice"): the marginal likelihood of all paths compatible with a
// partial annotation, its gradients, the constrained posteriors and the best allowed path.  Extends the call sites of the
// reference's third-party CRF (models/bert_model.py:464 ctor, :511 decode, :521 likelihood), which take one tag per
// position or none at all.
//   allowed int64 [B,S], read as an unsigned word: bit j set = tag j may be taken at that column.  The effective set is
//   A[b,t] = allowed[b,t] & (2^C - 1), and the FULL set where that is empty (0 = "no constraint", bits >= C ignored), so
//   every input has a finite answer and nothing is checked on the host.  mask is a prefix mask; len_b = its leading ones,
//   columns at or beyond len_b are never read (emissions, sets), end[] enters at column len_b - 1.
//   logZ_A[b] = log sum_{y: y_t in A[b,t]} exp score(y),   pllh[b] = logZ_A[b] - logZ[b].
// One wavefront per sentence, tag j on lane j, 1 <= C <= 64, 1 <= S <= 512; CT = 16, 32 or 64 is the unrolled width.
// The recursions run in the scaled linear domain of crf.hip / crf_wide.hip.  A constraint is a zeroed emission factor, so
// a constrained step costs what a free step costs, and the CONSTRAINED CHAIN (c = 0) AND THE FREE CHAIN (c = 1) RUN
// INTERLEAVED IN ONE WAVE through the same statements: they share the transition factors in registers, and each fills the
// issue slots the other's dependent chain leaves empty.  Two consequences that are part of the contract:
//   * a sentence whose sets are all full takes bit-identical values through both chains, so pllh = logZ_A - logZ is +0.0
//     and every gradient, formed as a DIFFERENCE FIRST (muA - mu, GA - G), is an exact zero.  Contraction is off in this
//     file -- the pragma below for the front end and -ffp-contract=off in build.py for the code generator, which under
//     the library's -ffp-contract=fast fuses a product into the subtraction it feeds whatever the pragma says -- and the
//     sums of products are explicit fmaf;
//   * the constrained chain takes its emission maximum over the allowed tags only: however far the allowed emissions lie
//     below the others, its factors have maximum 1.
// A step's C-term product is a lane broadcast through LDS (crf_wide.hip): every lane writes its value and reads the CT
// values back as ds_read_b128 against a column (forward) or row (backward) of E = exp(trans - tmax) held in registers.
// The normaliser comes out of the same broadcast (each lane adds the values it reads: bit-identical in every lane), so
// there is no cross-lane reduction on the serial path.
#include "common.h"

#pragma clang fp contract(off)

#include "crf_chain.h"  // (behind the pragma: lds_fence, prefix_len, trans_max, dot_sum, dot_dot, param_reduce, the dispatch)

namespace mtvaf {
namespace lat {

constexpr int CMAX = CRF_CHAIN_CMAX;
constexpr int SMAX = CRF_CHAIN_SMAX;

__device__ __forceinline__ uint64_t full_set(int C) { return C >= 64 ? ~0ull : (1ull << C) - 1ull; }
__device__ __forceinline__ uint64_t tag_set(const int64_t* __restrict__ arow, int t, uint64_t full) {
  const uint64_t a = (uint64_t)arow[t] & full;
  return a ? a : full;
}

// ---------------------------------------------------------------------------------------------
// forward, NCH chains (chain 0 constrained; chain 1, if present, free).  s is the scaled alpha; r = 1 / sum(s) is known one
// step late (it comes out of the broadcast that forms the next product) and is applied there:
//     dot_t[j] = sum_i s_{t-1}[i] E[i][j],   sp_t = dot_t r_t,   s_t = sp_t x_t,   x_t[j] = [j in A_t] exp(em_t[j] - mx_t),
//     alpha_t = K_t s_t,   log K_t = log K_{t-1} + tmax + mx_t - log r_t,   mx_t = max over the chain's set at t.
// Left for the backward: alpha_ws[c][b][t] = s_t r_{t+1} (sum 1), sp_ws[c][b][t] = sp_t (the predicted alpha on the scale
// of alpha_ws[t-1]), mx_ws[c][b][t] = mx_t.  The len - 1 logarithms are taken in parallel after the loop and summed in double.
// ---------------------------------------------------------------------------------------------
template <int CT, int NCH>
__global__ __launch_bounds__(64) void lat_fwd_kernel(const float* __restrict__ em, const int64_t* __restrict__ allowed,
                                                    const uint8_t* __restrict__ mask, const float* __restrict__ start,
                                                    const float* __restrict__ end, const float* __restrict__ trans,
                                                    float* __restrict__ alpha_ws, float* __restrict__ sp_ws,
                                                    float* __restrict__ mx_ws, float* __restrict__ pllh,
                                                    float* __restrict__ logz_a, float* __restrict__ logz, int B, int S, int C) {
  __shared__ __attribute__((aligned(16))) float bc[NCH][64];
  __shared__ uint64_t aw[SMAX];
  __shared__ float mxs[NCH][SMAX];
  __shared__ float rl[NCH][SMAX];
  const int b = blockIdx.x, j = threadIdx.x;
  const bool act = j < C;
  const uint64_t full = full_set(C);
  const int len = prefix_len(mask + (long)b * S, S, j);
  const float* emb = em + (long)b * S * C;
  const int64_t* arow = allowed + (long)b * S;
  for (int t = j; t < len; t += 64) {
    const uint64_t a = tag_set(arow, t, full);
    aw[t] = a;
    const float* e = emb + (long)t * C;
    float m0 = NEG, m1 = NEG;
    for (int i = 0; i < C; ++i) {
      const float v = e[i];
      m1 = fmaxf(m1, v);
      if ((a >> i) & 1) m0 = fmaxf(m0, v);
    }
    mxs[0][t] = m0;
    mx_ws[((long)0 * B + b) * S + t] = m0;
    if (NCH > 1) {
      mxs[1][t] = m1;
      mx_ws[((long)1 * B + b) * S + t] = m1;
    }
  }
  __syncthreads();
  const float tmax = trans_max(trans, C, j);
  float w[CT];  // column j of E
#pragma unroll
  for (int i = 0; i < CT; ++i) w[i] = (act && i < C) ? __expf(trans[i * C + j] - tmax) : 0.f;
  float s[NCH], c0[NCH];
  float* aw_c[NCH];
  float* sp_c[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const uint64_t A = c == 0 ? aw[0] : full;
    const bool ok = act && ((A >> j) & 1);
    const float a0 = ok ? start[j] + emb[j] : NEG;
    c0[c] = wave_max(a0);
    s[c] = ok ? __expf(a0 - c0[c]) : 0.f;
    aw_c[c] = alpha_ws + ((long)c * B + b) * S * CT + j;
    sp_c[c] = sp_ws + ((long)c * B + b) * S * CT + j;
  }
  float en = (len > 1 && act) ? emb[C + j] : 0.f;
  for (int t = 1; t < len; ++t) {
    const float et = en;
    if (t + 1 < len && act) en = emb[(long)(t + 1) * C + j];
    const uint64_t At = aw[t];
#pragma unroll
    for (int c = 0; c < NCH; ++c) bc[c][j] = s[c];
    lds_fence();
    float dot[NCH], sum[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) dot_sum<CT>(bc[c], w, dot[c], sum[c]);
    lds_fence();
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const uint64_t A = c == 0 ? At : full;
      const bool ok = act && ((A >> j) & 1);
      const float x = ok ? __expf(et - mxs[c][t]) : 0.f;
      const float r = __builtin_amdgcn_rcpf(sum[c]);
      const float sp = dot[c] * r;
      if (j < CT) {
        aw_c[c][(long)(t - 1) * CT] = s[c] * r;
        sp_c[c][(long)t * CT] = sp;
      }
      if (j == 0) rl[c][t] = r;
      s[c] = sp * x;
    }
  }
  double z[NCH];
  __syncthreads();
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const float r = __builtin_amdgcn_rcpf(wave_sum(s[c]));
    if (j < CT) aw_c[c][(long)(len - 1) * CT] = s[c] * r;
    // log sum_j s[j] exp(end[j]) in the log domain (once per sentence): s is 0 outside the last set
    const bool pos = act && s[c] > 0.f;
    const float v = pos ? __logf(s[c]) + end[j] : NEG;
    const float m = wave_max(v);
    const float fin = m + __logf(wave_sum(pos ? __expf(v - m) : 0.f));
    // the terms are float32; their sum over up to 511 columns is taken in double (once per sentence, off the serial path) so
    // that pllh, a difference of two such sums, keeps the accuracy of its terms and not that of their magnitude
    double lz = 0.0;
    for (int t = 1 + j; t < len; t += 64) lz += ((double)tmax + (double)mxs[c][t]) - (double)__logf(rl[c][t]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lz += __shfl_xor(lz, o, 64);
    z[c] = ((double)c0[c] + lz) + (double)fin;
  }
  if (j == 0) {
    if (logz_a) logz_a[b] = (float)z[0];
    if (NCH > 1) {
      if (logz) logz[b] = (float)z[NCH - 1];
      if (pllh) pllh[b] = (float)(z[0] - z[NCH - 1]);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// backward, t = len-1 .. 1, per chain:  u = x_t b_t,  d = sp_t . u,  ui_t = u / d,  b_{t-1} = (E u) / d  (so that
// alpha_ws[t-1] . b_{t-1} = 1),  node marginal mu_t = sp_t ui_t,  edge marginals xi_t[i][j] = alpha_ws[t-1][i] E[i][j] ui_t[j].
// u, sp_t and alpha_ws[t-1] go through one broadcast; lane j accumulates column j of G[i][j] = sum_t alpha_ws[t-1][i] ui_t[j].
//   MARG = false (NCH = 2): out = dem[b,t,:] = grad[b] (muA - mu), zeros at masked columns; partial[b] = [start C | end C |
//                           trans C*C] of (constrained - free) marginals, weighted by grad in lat_param_reduce_kernel.
//   MARG = true  (NCH = 1): out = muA itself; no edge marginals, no partials.
// ---------------------------------------------------------------------------------------------
template <int CT, int NCH, bool MARG>
__global__ __launch_bounds__(64) void lat_bwd_kernel(const float* __restrict__ grad, const float* __restrict__ em,
                                                    const int64_t* __restrict__ allowed, const uint8_t* __restrict__ mask,
                                                    const float* __restrict__ end, const float* __restrict__ trans,
                                                    const float* __restrict__ alpha_ws, const float* __restrict__ sp_ws,
                                                    const float* __restrict__ mx_ws, float* __restrict__ out,
                                                    float* __restrict__ partial, int B, int S, int C) {
  __shared__ __attribute__((aligned(16))) float bu[NCH][64];
  __shared__ __attribute__((aligned(16))) float bs[NCH][64];
  __shared__ __attribute__((aligned(16))) float ba[NCH][64];
  __shared__ uint64_t aw[SMAX];
  __shared__ float mxs[NCH][SMAX];
  const int b = blockIdx.x, j = threadIdx.x;
  const bool act = j < C, inct = j < CT;
  const uint64_t full = full_set(C);
  const int len = prefix_len(mask + (long)b * S, S, j);
  const float* emb = em + (long)b * S * C;
  const int64_t* arow = allowed + (long)b * S;
  for (int t = j; t < len; t += 64) {
    aw[t] = tag_set(arow, t, full);
#pragma unroll
    for (int c = 0; c < NCH; ++c) mxs[c][t] = mx_ws[((long)c * B + b) * S + t];
  }
  __syncthreads();
  const float tmax = trans_max(trans, C, j);
  float wr[CT];  // row j of E
#pragma unroll
  for (int i = 0; i < CT; ++i) wr[i] = (act && i < C) ? __expf(trans[j * C + i] - tmax) : 0.f;
  const float g = MARG ? 1.f : grad[b];
  float G[MARG ? 1 : NCH][MARG ? 1 : CT];
  if constexpr (!MARG) {
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
      for (int i = 0; i < CT; ++i) G[c][i] = 0.f;
  }
  const float* al_c[NCH];
  const float* sp_c[NCH];
  float bt[NCH], pen[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    al_c[c] = alpha_ws + ((long)c * B + b) * S * CT + j;
    sp_c[c] = sp_ws + ((long)c * B + b) * S * CT + j;
    const uint64_t A = c == 0 ? aw[len - 1] : full;
    const bool ok = act && ((A >> j) & 1);
    const float m = wave_max(ok ? end[j] : NEG);
    bt[c] = ok ? __expf(end[j] - m) : 0.f;  // beta of the last column, any positive scale
    const float pe = (inct ? al_c[c][(long)(len - 1) * CT] : 0.f) * bt[c];
    pen[c] = pe * __builtin_amdgcn_rcpf(wave_sum(pe));
  }
  float* ob = out + (long)b * S * C;
  float en = (len > 1 && act) ? emb[(long)(len - 1) * C + j] : 0.f;
  float spn[NCH], aln[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    spn[c] = (len > 1 && inct) ? sp_c[c][(long)(len - 1) * CT] : 0.f;
    aln[c] = (len > 1 && inct) ? al_c[c][(long)(len - 2) * CT] : 0.f;
  }
  for (int t = len - 1; t >= 1; --t) {
    const float et = en;
    float spv[NCH], alv[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      spv[c] = spn[c];
      alv[c] = aln[c];
    }
    if (t >= 2) {
      if (act) en = emb[(long)(t - 1) * C + j];
      if (inct) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          spn[c] = sp_c[c][(long)(t - 1) * CT];
          aln[c] = al_c[c][(long)(t - 2) * CT];
        }
      }
    }
    const uint64_t At = aw[t];
    float u[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const uint64_t A = c == 0 ? At : full;
      const bool ok = act && ((A >> j) & 1);
      const float x = ok ? __expf(et - mxs[c][t]) : 0.f;
      u[c] = x * bt[c];
      bu[c][j] = u[c];
      bs[c][j] = spv[c];
      if constexpr (!MARG) ba[c][j] = alv[c];
    }
    lds_fence();
    float mu[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      float eu, d;
      dot_dot<CT>(bu[c], bs[c], wr, eu, d);
      const float r = __builtin_amdgcn_rcpf(d);
      const float ui = u[c] * r;
      mu[c] = spv[c] * ui;
      bt[c] = eu * r;
      if constexpr (!MARG) {
        const f4* a4 = reinterpret_cast<const f4*>(ba[c]);
#pragma unroll
        for (int q = 0; q < CT / 4; ++q) {
          const f4 a = a4[q];
          G[c][4 * q] = __builtin_fmaf(a.x, ui, G[c][4 * q]);
          G[c][4 * q + 1] = __builtin_fmaf(a.y, ui, G[c][4 * q + 1]);
          G[c][4 * q + 2] = __builtin_fmaf(a.z, ui, G[c][4 * q + 2]);
          G[c][4 * q + 3] = __builtin_fmaf(a.w, ui, G[c][4 * q + 3]);
        }
      }
    }
    lds_fence();
    if (act) ob[(long)t * C + j] = MARG ? mu[0] : g * (mu[0] - mu[NCH - 1]);
  }
  float p0n[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const float p0 = (inct ? al_c[c][0] : 0.f) * bt[c];
    p0n[c] = p0 * __builtin_amdgcn_rcpf(wave_sum(p0));
  }
  if (act) ob[j] = MARG ? p0n[0] : g * (p0n[0] - p0n[NCH - 1]);
  for (int idx = len * C + j; idx < S * C; idx += 64) ob[idx] = 0.f;  // masked columns: exact zeros
  if constexpr (!MARG) {
    if (act) {
      float* pp = partial + (long)b * (2 * C + C * C);
      pp[j] = p0n[0] - p0n[NCH - 1];
      pp[C + j] = pen[0] - pen[NCH - 1];
#pragma unroll
      for (int i = 0; i < CT; ++i)
        if (i < C) pp[2 * C + i * C + j] = (G[0][i] - G[NCH - 1][i]) * __expf(trans[i * C + j] - tmax);
    }
  }
}

// d[i] = sum_b grad[b] partial[b][i], overwritten or accumulated (crf_chain.h; compiled here with contraction off)
__global__ void lat_param_reduce_kernel(const float* __restrict__ partial, const float* __restrict__ grad, int B, int C,
                                        float* __restrict__ dstart, float* __restrict__ dend, float* __restrict__ dtrans,
                                        int accumulate) {
  param_reduce(partial, grad, B, C, dstart, dend, dtrans, accumulate);
}

// ---------------------------------------------------------------------------------------------
// Viterbi over the allowed paths, mtvaf_crf_viterbi's order of additions: score_t[j] = max_i (score_{t-1}[i] + trans[i][j])
// + em_t[j], the LOWEST i attaining the maximum; at the end max_j (score[j] + end[j]), the lowest j.  A disallowed tag
// carries -inf, so it is never a maximum and never a back-pointer; with full sets nothing is -inf and the result is that
// kernel's bit for bit.  Back-pointers: one byte per (column, tag) in LDS.
// ---------------------------------------------------------------------------------------------
template <int CT>
__global__ __launch_bounds__(64) void lat_viterbi_kernel(const float* __restrict__ em, const int64_t* __restrict__ allowed,
                                                        const uint8_t* __restrict__ mask, const float* __restrict__ start,
                                                        const float* __restrict__ end, const float* __restrict__ trans,
                                                        int32_t* __restrict__ tags_out, int32_t* __restrict__ lens_out,
                                                        float* __restrict__ score_out, int S, int C) {
  __shared__ __attribute__((aligned(16))) float bc[64];
  __shared__ uint64_t aw[SMAX];
  __shared__ int path[SMAX];
  extern __shared__ uint8_t lat_bp[];  // [S][CT]
  const float NINF = -__builtin_inff();
  const int b = blockIdx.x, j = threadIdx.x;
  const bool act = j < C;
  const uint64_t full = full_set(C);
  const int len = prefix_len(mask + (long)b * S, S, j);
  const float* emb = em + (long)b * S * C;
  const int64_t* arow = allowed + (long)b * S;
  for (int t = j; t < len; t += 64) aw[t] = tag_set(arow, t, full);
  __syncthreads();
  float tc[CT];  // column j of trans; -inf: a padding candidate never wins
#pragma unroll
  for (int i = 0; i < CT; ++i) tc[i] = (act && i < C) ? trans[i * C + j] : NINF;
  float score = (act && ((aw[0] >> j) & 1)) ? start[j] + emb[j] : NINF;
  float en = (len > 1 && act) ? emb[C + j] : 0.f;
  for (int t = 1; t < len; ++t) {
    const float et = en;
    if (t + 1 < len && act) en = emb[(long)(t + 1) * C + j];
    const bool ok = act && ((aw[t] >> j) & 1);
    bc[j] = score;
    lds_fence();
    const f4* b4 = reinterpret_cast<const f4*>(bc);
    float best = NINF;
    int bi = 0;
#pragma unroll
    for (int q = 0; q < CT / 4; ++q) {
      const f4 x = b4[q];
      const float v0 = x.x + tc[4 * q], v1 = x.y + tc[4 * q + 1], v2 = x.z + tc[4 * q + 2], v3 = x.w + tc[4 * q + 3];
      if (v0 > best) { best = v0; bi = 4 * q; }
      if (v1 > best) { best = v1; bi = 4 * q + 1; }
      if (v2 > best) { best = v2; bi = 4 * q + 2; }
      if (v3 > best) { best = v3; bi = 4 * q + 3; }
    }
    lds_fence();
    score = ok ? best + et : NINF;
    if (j < CT) lat_bp[t * CT + j] = (uint8_t)bi;
  }
  float fin = act ? score + end[j] : NINF;
  int idx = act ? j : CMAX;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(fin, o, 64);
    const int oi = __shfl_xor(idx, o, 64);
    if (ov > fin || (ov == fin && oi < idx)) {
      fin = ov;
      idx = oi;
    }
  }
  __syncthreads();
  int cur = __builtin_amdgcn_readfirstlane(idx);
  cur = cur < C ? cur : 0;
  if (j == 0) {
    path[len - 1] = cur;
    for (int t = len - 1; t >= 1; --t) {
      cur = lat_bp[t * CT + cur];
      path[t - 1] = cur;
    }
  }
  __syncthreads();
  int32_t* o = tags_out + (long)b * S;
  for (int t = j; t < S; t += 64) o[t] = t < len ? path[t] : -1;
  if (j == 0) {
    lens_out[b] = len;
    if (score_out) score_out[b] = fin;
  }
}

// workspace, in floats, CT = 16, 32 or 64:  alpha [2,B,S,CT] | sp [2,B,S,CT] | mx [2,B,S] | partials [B, 2C + C*C]
struct Ws {
  float *alpha, *sp, *mx, *partial;
};
inline size_t ws_floats(int B, int S, int C) {
  const size_t n = (size_t)B * S;
  return 4 * n * width(C) + 2 * n + (size_t)B * (2 * C + C * C);
}
inline Ws ws_of(void* p, int B, int S, int C) {
  const size_t n = (size_t)B * S;
  Ws w;
  w.alpha = (float*)p;
  w.sp = w.alpha + 2 * n * width(C);
  w.mx = w.sp + 2 * n * width(C);
  w.partial = w.mx + 2 * n;
  return w;
}

template <int NCH>
int launch_fwd(const float* em, const int64_t* allowed, const uint8_t* mask, const float* start, const float* end,
               const float* trans, const Ws& w, float* pllh, float* logz_a, float* logz, int B, int S, int C, hipStream_t st) {
#define LAT_FWD(CT)                                                                                                    \
  hipLaunchKernelGGL((lat_fwd_kernel<CT, NCH>), dim3(B), dim3(64), 0, st, em, allowed, mask, start, end, trans, w.alpha, \
                     w.sp, w.mx, pllh, logz_a, logz, B, S, C)
  CRF_CHAIN_DISPATCH(C, LAT_FWD)
#undef LAT_FWD
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

template <int NCH, bool MARG>
int launch_bwd(const float* grad, const float* em, const int64_t* allowed, const uint8_t* mask, const float* end,
               const float* trans, const Ws& w, float* out, int B, int S, int C, hipStream_t st) {
#define LAT_BWD(CT)                                                                                                    \
  hipLaunchKernelGGL((lat_bwd_kernel<CT, NCH, MARG>), dim3(B), dim3(64), 0, st, grad, em, allowed, mask, end, trans,    \
                     w.alpha, w.sp, w.mx, out, w.partial, B, S, C)
  CRF_CHAIN_DISPATCH(C, LAT_BWD)
#undef LAT_BWD
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

}  // namespace lat
}  // namespace mtvaf

using namespace mtvaf;

extern "C" {

size_t mtvaf_crf_lattice_workspace_bytes(int B, int S, int C) {
  return bad_shape(B, S, C) ? 0 : lat::ws_floats(B, S, C) * sizeof(float);
}

// pllh [B] = logZ_A - logZ; logz_a [B], logz [B] nullable.  One launch; the workspace keeps what lattice_bwd reads.
int mtvaf_crf_lattice_fwd(const float* emissions, const int64_t* allowed, const uint8_t* mask, const float* start,
                          const float* end, const float* trans, float* pllh, float* logz_a, float* logz, int B, int S,
                          int C, void* workspace, size_t workspace_bytes, hipStream_t st) {
  if (bad_shape(B, S, C)) return MTVAF_ERR_SHAPE;
  if (workspace_bytes < mtvaf_crf_lattice_workspace_bytes(B, S, C)) return MTVAF_ERR_WORKSPACE;
  return lat::launch_fwd<2>(emissions, allowed, mask, start, end, trans, lat::ws_of(workspace, B, S, C), pllh, logz_a, logz,
                            B, S, C, st);
}

// gradients of sum_b grad[b] pllh[b]: demissions[b,t,:] = grad[b] (muA - mu), exact zeros at masked columns; the parameter
// gradients overwritten or accumulated.  Two launches (the recursion, the reduction of the per-sentence partials).
int mtvaf_crf_lattice_bwd(const float* grad, const float* emissions, const int64_t* allowed, const uint8_t* mask,
                          const float* start, const float* end, const float* trans, float* demissions, float* dstart,
                          float* dend, float* dtrans, int accumulate, int B, int S, int C, void* workspace,
                          size_t workspace_bytes, hipStream_t st) {
  (void)start;  // (enters through the workspace's alphas)
  if (bad_shape(B, S, C)) return MTVAF_ERR_SHAPE;
  if (workspace_bytes < mtvaf_crf_lattice_workspace_bytes(B, S, C)) return MTVAF_ERR_WORKSPACE;
  const lat::Ws w = lat::ws_of(workspace, B, S, C);
  if (int rc = lat::launch_bwd<2, false>(grad, emissions, allowed, mask, end, trans, w, demissions, B, S, C, st)) return rc;
  const int n = 2 * C + C * C;
  hipLaunchKernelGGL(lat::lat_param_reduce_kernel, dim3((n + 255) / 256), dim3(256), 0, st, w.partial, grad, B, C, dstart,
                     dend, dtrans, accumulate);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

// marg [B,S,C] = the constrained posteriors muA: exact zeros at disallowed tags and masked columns; logz_a [B] nullable.
// Two launches, the constrained chain alone.  Overwrites the workspace of a preceding lattice_fwd.
int mtvaf_crf_lattice_marginals(const float* emissions, const int64_t* allowed, const uint8_t* mask, const float* start,
                                const float* end, const float* trans, float* marg, float* logz_a, int B, int S, int C,
                                void* workspace, size_t workspace_bytes, hipStream_t st) {
  if (bad_shape(B, S, C)) return MTVAF_ERR_SHAPE;
  if (workspace_bytes < mtvaf_crf_lattice_workspace_bytes(B, S, C)) return MTVAF_ERR_WORKSPACE;
  const lat::Ws w = lat::ws_of(workspace, B, S, C);
  if (int rc = lat::launch_fwd<1>(emissions, allowed, mask, start, end, trans, w, nullptr, logz_a, nullptr, B, S, C, st))
    return rc;
  return lat::launch_bwd<1, true>(nullptr, emissions, allowed, mask, end, trans, w, marg, B, S, C, st);
}

// tags_out int32 [B,S] (best allowed path, -1 behind len_b), lens_out int32 [B], score_out [B] (nullable) its
// unnormalised score.  One launch, no workspace.
int mtvaf_crf_lattice_viterbi(const float* emissions, const int64_t* allowed, const uint8_t* mask, const float* start,
                              const float* end, const float* trans, int32_t* tags_out, int32_t* lens_out, float* score_out,
                              int B, int S, int C, hipStream_t st) {
  if (bad_shape(B, S, C)) return MTVAF_ERR_SHAPE;
#define LAT_VIT(CT)                                                                                                    \
  hipLaunchKernelGGL(lat::lat_viterbi_kernel<CT>, dim3(B), dim3(64), (size_t)S * CT, st, emissions, allowed, mask, start, \
                     end, trans, tags_out, lens_out, score_out, S, C)
  CRF_CHAIN_DISPATCH(C, LAT_VIT)
#undef LAT_VIT
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

}  // extern "C"
