// Linear-chain CRF: the expected value of a PATH cost with a term on every edge, under the chain's posterior, and its gradients.
// Extends csrc/crf_risk.hip (column-additive costs only) by one term per previous tag; with it come the sequence entropy, the
// KL divergence between two chains, and the edge marginals sum_t xi_t(i,j) as an output.
//   cost fp32 [B,S,C] or NULL, ecost fp32 [C,C] or NULL (NULL reads as zeros);
//   W(y) = sum_{t < len} cost[b,t,y_t] + sum_{1 <= t < len} ecost[y_{t-1},y_t],   R[b] = E_{y ~ p(.|x_b)} W(y).
//   With a_t(j) = E[W of columns 0..t | y_t = j], b_t(i) = E[W of columns t+1.. and the edge into t+1 | y_t = i]:
//     dR/dem[t,c] = m_t(c) (a_t(c) + b_t(c) - R),
//     dR/dtrans[i,j] = sum_{t>=1} xi_t(i,j) (a_{t-1}(i) + ecost[i,j] + cost[t,j] + b_t(j) - R),
//     dR/dstart = dR/dem[0], dR/dend = dR/dem[len-1], dR/dcost[t,c] = m_t(c), dR/decost[i,j] = sum_{t>=1} xi_t(i,j).
//   The backward writes the gradients of sum_b grad[b] R[b] + gz[b] logZ[b] (gz NULL: zeros): the gz term adds gz m_t(c) to
//   dem, gz sum_t xi_t to dtrans and gz times the end-point marginals to dstart / dend.
//   mask is a prefix mask; len_b = its leading ones; cost and emissions at or beyond len_b are never read.
// One wavefront per sentence, tag j on lane j, 1 <= C <= 64, 1 <= S <= 512; CT = 16, 32 or 64 is the unrolled width; EC says
// whether ecost is given.  The scaled linear domain, the LDS lane broadcast, the two interleaved chains and the CENTRING are
// those of crf_risk.hip (its header has the derivation; the helpers both files use are in crf_chain.h).  With
// E = exp(trans - tmax) and F = E o ecost the edge term enters in four places:
//   forward    at_t(j) = cost_t(j) + ((abar_{t-1} o ac_{t-1}) E + abar_{t-1} F)(j) / sp_t(j):  one more FMA per previous tag;
//   backward   eq = E q + F u  (one more FMA per next tag),  dq = sum_j (sp_t(j) q(j) + spf_t(j) u(j))  with spf_t = abar_{t-1} F
//              kept by the forward (so the centring constant still comes out of the broadcast, bit-identical in every lane,
//              with no cross-lane reduction on the serial path);
//   gradient   N = sum_t outer(abar_{t-1}, ui_t) beside G:  dtrans = G o E + N o F,  decost = N o E  (= sum_t xi_t);
//              G and k are those of crf_risk.hip: the xi_t-weighted mean of the bracket is still dbar_t + mean_t, because
//              at_t now contains the edge term;
//   R = sum_t mean_t + sum_j p(y_last = j) ac_last(j), summed in double.
// Registers: the forward keeps column j of E in registers and reads column j of F from LDS ([i][j], lanes on consecutive
// words); the backward keeps G and N in registers (2 CT) and reads row i of E and of F from LDS ([i][CT + 1]: lane i on bank
// i + j, conflict-free), which at CT = 64 is 2 x 16.25 KB.
//
// Exact zeros (none relies on the contraction mode):
//   * cost and ecost both zero (or NULL) on the live columns: F is +-0.0, so at, mean, ac, bc, bmean, d, dbar, k, G and N o F
//     are zeros whose sums with +0.0 are +0.0: R == +0.0 and every cost-covariance gradient is +0.0 whatever the sign of grad;
//   * grad[b] == 0 and gz[b] == 0: that sentence's dem, dcost and shares of the parameter gradients are zeros (x + 0.0);
//   * masked columns of dem and dcost are written as +0.0.
#include "crf_chain.h"

namespace mtvaf {
namespace path {

constexpr int SMAX = CRF_CHAIN_SMAX;

// sum_i v[i] f[i * stride] over a broadcast row and this lane's own strided LDS values.  A real loop over 16 tags at a time
// (nothing here indexes a register array): unrolled in full, the compiler issues every load first and spills around them.
template <int CT>
__device__ __forceinline__ float dot_lds(const float* row, const float* f, int stride) {
  const f4* r4 = reinterpret_cast<const f4*>(row);
  float d0 = 0.f, d1 = 0.f, d2 = 0.f, d3 = 0.f;
#pragma clang loop unroll(disable)
  for (int q0 = 0; q0 < CT / 4; q0 += 4) {
#pragma unroll
    for (int q = q0; q < q0 + 4; ++q) {
      const f4 x = r4[q];
      d0 = __builtin_fmaf(x.x, f[(4 * q) * stride], d0);
      d1 = __builtin_fmaf(x.y, f[(4 * q + 1) * stride], d1);
      d2 = __builtin_fmaf(x.z, f[(4 * q + 2) * stride], d2);
      d3 = __builtin_fmaf(x.w, f[(4 * q + 3) * stride], d3);
    }
  }
  return (d0 + d1) + (d2 + d3);
}

// ---------------------------------------------------------------------------------------------
// forward: crf_risk.hip's, with  dotf_t[j] = sum_i s_{t-1}[i] F[i][j]  out of the same broadcast:
//     at_t[j] = cost_t[j] + ((dotu_t[j] + dotf_t[j]) / dot_t[j] - mean_{t-1}),   spf_ws[b][t] = dotf_t r  (= abar_{t-1} F).
// ---------------------------------------------------------------------------------------------
template <int CT, bool EC>
__global__ __launch_bounds__(64) void path_fwd_kernel(const float* __restrict__ em, const float* __restrict__ cost,
                                                     const float* __restrict__ ecost, const uint8_t* __restrict__ mask,
                                                     const float* __restrict__ start, const float* __restrict__ end,
                                                     const float* __restrict__ trans, float* __restrict__ alpha_ws,
                                                     float* __restrict__ sp_ws, float* __restrict__ ac_ws,
                                                     float* __restrict__ spf_ws, float* __restrict__ mx_ws,
                                                     float* __restrict__ mean_ws, float* __restrict__ risk_out,
                                                     float* __restrict__ logz_out, int S, int C) {
  __shared__ __attribute__((aligned(16))) float bc[2][64];
  __shared__ float mxs[SMAX];
  __shared__ float rl[SMAX];
  __shared__ float mns[SMAX];
  __shared__ float fl[EC ? CT * CT : 1];  // F, [i][j]
  const int b = blockIdx.x, j = threadIdx.x;
  const bool act = j < C, inct = j < CT;
  const int len = prefix_len(mask + (long)b * S, S, j);
  const float* emb = em + (long)b * S * C;
  const float* cb = cost ? cost + (long)b * S * C : nullptr;
  const float tmax = trans_max(trans, C, j);
  for (int t = j; t < len; t += 64) {
    const float* e = emb + (long)t * C;
    float m = NEG;
    for (int i = 0; i < C; ++i) m = fmaxf(m, e[i]);
    mxs[t] = m;
    mx_ws[(long)b * S + t] = m;
  }
  if constexpr (EC) {
    for (int idx = j; idx < CT * CT; idx += 64) {
      const int i = idx / CT, k = idx % CT;
      fl[idx] = (i < C && k < C) ? __expf(trans[i * C + k] - tmax) * ecost[i * C + k] : 0.f;
    }
  }
  __syncthreads();
  float w[CT];  // column j of E
#pragma unroll
  for (int i = 0; i < CT; ++i) w[i] = (act && i < C) ? __expf(trans[i * C + j] - tmax) : 0.f;
  const float* fcol = fl + (inct ? j : 0);
  const float a0 = act ? start[j] + emb[j] : NEG;
  const float c0 = wave_max(a0);
  float s = act ? __expf(a0 - c0) : 0.f;
  float at = (act && cb) ? cb[j] : 0.f;
  float* al_p = alpha_ws + (long)b * S * CT + j;
  float* sp_p = sp_ws + (long)b * S * CT + j;
  float* ac_p = ac_ws + (long)b * S * CT + j;
  float* sf_p = spf_ws + (long)b * S * CT + j;
  float en = (len > 1 && act) ? emb[C + j] : 0.f;
  float cn = (len > 1 && act && cb) ? cb[C + j] : 0.f;
  for (int t = 1; t < len; ++t) {
    const float et = en, ct = cn;
    if (t + 1 < len && act) {
      en = emb[(long)(t + 1) * C + j];
      if (cb) cn = cb[(long)(t + 1) * C + j];
    }
    bc[0][j] = s;
    bc[1][j] = s * at;
    lds_fence();
    float dot, sum, dotu, sumu, dotf = 0.f;
    dot_sum<CT>(bc[0], w, dot, sum);
    dot_sum<CT>(bc[1], w, dotu, sumu);
    if constexpr (EC) dotf = dot_lds<CT>(bc[0], fcol, CT);
    lds_fence();
    const float x = act ? __expf(et - mxs[t]) : 0.f;
    const float r = __builtin_amdgcn_rcpf(sum);
    const float mean = sumu * r;
    const float sp = dot * r;
    if (inct) {
      al_p[(long)(t - 1) * CT] = s * r;
      sp_p[(long)t * CT] = sp;
      ac_p[(long)(t - 1) * CT] = at - mean;
      if constexpr (EC) sf_p[(long)t * CT] = dotf * r;
    }
    if (j == 0) {
      rl[t] = r;
      mns[t - 1] = mean;
    }
    at = (act && dot > 0.f) ? ct + ((dotu + dotf) * __builtin_amdgcn_rcpf(dot) - mean) : 0.f;
    s = sp * x;
  }
  const float r = __builtin_amdgcn_rcpf(wave_sum(s));
  const float mean = wave_sum(s * at) * r;
  const float ac = at - mean;
  if (inct) {
    al_p[(long)(len - 1) * CT] = s * r;
    ac_p[(long)(len - 1) * CT] = ac;
  }
  if (j == 0) mns[len - 1] = mean;
  __syncthreads();
  // log sum_j s[j] exp(end[j]) in the log domain, and the posterior of the last tag (once per sentence)
  const bool pos = act && s > 0.f;
  const float v = pos ? __logf(s) + end[j] : NEG;
  const float m = wave_max(v);
  const float pe = pos ? __expf(v - m) : 0.f;
  const float pes = wave_sum(pe);
  const float fin = m + __logf(pes);
  const float rlast = wave_sum(pe * ac) * __builtin_amdgcn_rcpf(pes);
  double lz = 0.0, rs = 0.0;
  for (int t = j; t < len; t += 64) {
    const float mt = mns[t];
    mean_ws[(long)b * S + t] = mt;
    rs += (double)mt;
    if (t >= 1) lz += ((double)tmax + (double)mxs[t]) - (double)__logf(rl[t]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lz += __shfl_xor(lz, o, 64);
    rs += __shfl_xor(rs, o, 64);
  }
  if (j == 0) {
    risk_out[b] = (float)(rs + (double)rlast);
    if (logz_out) logz_out[b] = (float)(((double)c0 + lz) + (double)fin);
  }
}

// ---------------------------------------------------------------------------------------------
// backward, t = len-1 .. 1: crf_risk.hip's, with u, sp_t, q = u (cost_t + bh) and spf_t through one broadcast, from which
// every lane i takes (rows i of E and F from LDS)
//     eu = sum_j E[i][j] u[j],  d = sum_j sp_t[j] u[j],  eq = sum_j (E[i][j] q[j] + F[i][j] u[j]),
//     dq = sum_j (sp_t[j] q[j] + spf_t[j] u[j]);
// lane j accumulates column j of G (as there) and of N[i][j] = sum_t alpha_ws[t-1][i] ui_t[j].
//   dem[b,t,:] = g mu_t (d_t - dbar_t) + gz mu_t,  dcost[b,t,:] = g mu_t (if asked),  zeros at masked columns;
//   partial[b] = [dR/dstart C | dR/dend C | p(y_0) C | p(y_last) C | G o E + N o F  C*C | N o E  C*C], weighted by grad and gz
//   in path_param_reduce_kernel.
// ---------------------------------------------------------------------------------------------
template <int CT, bool EC>
__global__ __launch_bounds__(64) void path_bwd_kernel(const float* __restrict__ grad, const float* __restrict__ gz,
                                                     const float* __restrict__ em, const float* __restrict__ cost,
                                                     const float* __restrict__ ecost, const uint8_t* __restrict__ mask,
                                                     const float* __restrict__ end, const float* __restrict__ trans,
                                                     const float* __restrict__ alpha_ws, const float* __restrict__ sp_ws,
                                                     const float* __restrict__ ac_ws, const float* __restrict__ spf_ws,
                                                     const float* __restrict__ mx_ws, const float* __restrict__ mean_ws,
                                                     float* __restrict__ dem, float* __restrict__ dcost,
                                                     float* __restrict__ partial, int S, int C) {
  constexpr int LD = CT + 1;
  __shared__ __attribute__((aligned(16))) float bu[64];
  __shared__ __attribute__((aligned(16))) float bs[64];
  __shared__ __attribute__((aligned(16))) float bq[64];
  __shared__ __attribute__((aligned(16))) float ba[64];
  __shared__ __attribute__((aligned(16))) float bp[64];
  __shared__ __attribute__((aligned(16))) float bf[64];
  __shared__ float mxs[SMAX];
  __shared__ float mns[SMAX];
  __shared__ float el[CT * LD];           // E, [i][LD]
  __shared__ float fl[EC ? CT * LD : 1];  // F, [i][LD]
  const int b = blockIdx.x, j = threadIdx.x;
  const bool act = j < C, inct = j < CT;
  const int len = prefix_len(mask + (long)b * S, S, j);
  const float* emb = em + (long)b * S * C;
  const float* cb = cost ? cost + (long)b * S * C : nullptr;
  const float tmax = trans_max(trans, C, j);
  for (int t = j; t < len; t += 64) {
    mxs[t] = mx_ws[(long)b * S + t];
    mns[t] = mean_ws[(long)b * S + t];
  }
  for (int idx = j; idx < CT * CT; idx += 64) {
    const int i = idx / CT, k = idx % CT;
    const bool in = i < C && k < C;
    const float e = in ? __expf(trans[i * C + k] - tmax) : 0.f;
    el[i * LD + k] = e;
    if constexpr (EC) fl[i * LD + k] = in ? e * ecost[i * C + k] : 0.f;
  }
  __syncthreads();
  const float* erow = el + (inct ? j : 0) * LD;
  const float* frow = fl + (EC && inct ? j : 0) * LD;
  const float g = grad[b];
  const float gzb = gz ? gz[b] : 0.f;
  float G[CT], N[CT];
#pragma unroll
  for (int i = 0; i < CT; ++i) {
    G[i] = 0.f;
    N[i] = 0.f;
  }
  const float* al_p = alpha_ws + (long)b * S * CT + j;
  const float* sp_p = sp_ws + (long)b * S * CT + j;
  const float* ac_p = ac_ws + (long)b * S * CT + j;
  const float* sf_p = spf_ws + (long)b * S * CT + j;
  const float em_ = wave_max(act ? end[j] : NEG);
  float bt = act ? __expf(end[j] - em_) : 0.f;  // beta of the last column, any positive scale
  float bh = 0.f;                               // bc of the last column
  float* ob = dem + (long)b * S * C;
  float* oc = dcost ? dcost + (long)b * S * C : nullptr;
  float acur = inct ? ac_p[(long)(len - 1) * CT] : 0.f;  // ac of the column being written
  float dend_v = 0.f, pend_v = 0.f;
  float en = (len > 1 && act) ? emb[(long)(len - 1) * C + j] : 0.f;
  float cn = (len > 1 && act && cb) ? cb[(long)(len - 1) * C + j] : 0.f;
  float spn = (len > 1 && inct) ? sp_p[(long)(len - 1) * CT] : 0.f;
  float sfn = (EC && len > 1 && inct) ? sf_p[(long)(len - 1) * CT] : 0.f;
  float aln = (len > 1 && inct) ? al_p[(long)(len - 2) * CT] : 0.f;
  float acn = (len > 1 && inct) ? ac_p[(long)(len - 2) * CT] : 0.f;
  for (int t = len - 1; t >= 1; --t) {
    const float et = en, ct = cn, spv = spn, sfv = sfn, alv = aln, acv = acn;
    if (t >= 2) {
      if (act) {
        en = emb[(long)(t - 1) * C + j];
        if (cb) cn = cb[(long)(t - 1) * C + j];
      }
      if (inct) {
        spn = sp_p[(long)(t - 1) * CT];
        if constexpr (EC) sfn = sf_p[(long)(t - 1) * CT];
        aln = al_p[(long)(t - 2) * CT];
        acn = ac_p[(long)(t - 2) * CT];
      }
    }
    const float x = act ? __expf(et - mxs[t]) : 0.f;
    const float u = x * bt;
    bu[j] = u;
    bs[j] = spv;
    bq[j] = u * (ct + bh);
    ba[j] = alv;
    bp[j] = alv * acv;
    if constexpr (EC) bf[j] = sfv;
    lds_fence();
    float eu, d, eq, dq;
    {
      const f4* u4 = reinterpret_cast<const f4*>(bu);
      const f4* s4 = reinterpret_cast<const f4*>(bs);
      const f4* q4 = reinterpret_cast<const f4*>(bq);
      const f4* f4p = reinterpret_cast<const f4*>(bf);
      float eu_[4] = {0.f, 0.f, 0.f, 0.f}, d_[4] = {0.f, 0.f, 0.f, 0.f}, eq_[4] = {0.f, 0.f, 0.f, 0.f},
            dq_[4] = {0.f, 0.f, 0.f, 0.f};
#pragma clang loop unroll(disable)
      for (int q0 = 0; q0 < CT / 4; q0 += 4) {  // (a real loop over 16 tags at a time, as dot_lds)
#pragma unroll
        for (int q = q0; q < q0 + 4; ++q) {
          const f4 uv = u4[q], sv = s4[q], qv = q4[q];
          f4 fv = {0.f, 0.f, 0.f, 0.f};
          if constexpr (EC) fv = f4p[q];
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const float e = erow[4 * q + c];
            eu_[c] = __builtin_fmaf(e, uv[c], eu_[c]);
            d_[c] = __builtin_fmaf(sv[c], uv[c], d_[c]);
            eq_[c] = __builtin_fmaf(e, qv[c], eq_[c]);
            dq_[c] = __builtin_fmaf(sv[c], qv[c], dq_[c]);
            if constexpr (EC) {
              eq_[c] = __builtin_fmaf(frow[4 * q + c], uv[c], eq_[c]);
              dq_[c] = __builtin_fmaf(fv[c], uv[c], dq_[c]);
            }
          }
        }
      }
      eu = (eu_[0] + eu_[1]) + (eu_[2] + eu_[3]);
      d = (d_[0] + d_[1]) + (d_[2] + d_[3]);
      eq = (eq_[0] + eq_[1]) + (eq_[2] + eq_[3]);
      dq = (dq_[0] + dq_[1]) + (dq_[2] + dq_[3]);
    }
    const float r = __builtin_amdgcn_rcpf(d);
    const float ui = u * r;
    const float mu = spv * ui;
    bt = eu * r;
    const float dv = acur + bh;
    const float dbar = wave_sum(mu * dv);
    const float val = mu * (dv - dbar);
    const float k = ui * (((ct + bh) - dbar) - mns[t]);
    const f4* a4 = reinterpret_cast<const f4*>(ba);
    const f4* p4 = reinterpret_cast<const f4*>(bp);
#pragma unroll
    for (int q = 0; q < CT / 4; ++q) {
      if (q % 4 == 0) __builtin_amdgcn_sched_barrier(0);  // (16 tags' loads in flight at a time: G and N hold 2 CT registers)
      const f4 a = a4[q], p = p4[q];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        G[4 * q + c] = __builtin_fmaf(a[c], k, __builtin_fmaf(p[c], ui, G[4 * q + c]));
        N[4 * q + c] = __builtin_fmaf(a[c], ui, N[4 * q + c]);
      }
    }
    lds_fence();
    bh = (act && eu > 0.f) ? eq * __builtin_amdgcn_rcpf(eu) - dq * r : 0.f;
    if (t == len - 1) {
      dend_v = val;
      pend_v = mu;
    }
    acur = acv;
    if (act) {
      ob[(long)t * C + j] = (g * val + gzb * mu) + 0.f;  // (+ 0.f: a zero is written as +0.0 whatever the signs)
      if (oc) oc[(long)t * C + j] = g * mu + 0.f;
    }
  }
  const float p0 = (inct ? al_p[0] : 0.f) * bt;
  const float p0n = p0 * __builtin_amdgcn_rcpf(wave_sum(p0));
  const float dv = acur + bh;
  const float dbar = wave_sum(p0n * dv);
  const float val = p0n * (dv - dbar);
  if (len == 1) {
    dend_v = val;
    pend_v = p0n;
  }
  if (act) {
    ob[j] = (g * val + gzb * p0n) + 0.f;
    if (oc) oc[j] = g * p0n + 0.f;
  }
  for (int idx = len * C + j; idx < S * C; idx += 64) {  // masked columns: exact zeros
    ob[idx] = 0.f;
    if (oc) oc[idx] = 0.f;
  }
  if (act) {
    float* pp = partial + (long)b * (4 * C + 2 * C * C);
    pp[j] = val;
    pp[C + j] = dend_v;
    pp[2 * C + j] = p0n;
    pp[3 * C + j] = pend_v;
    float* t1 = pp + 4 * C;
    float* t2 = t1 + C * C;
#pragma unroll
    for (int i = 0; i < CT; ++i)
      if (i < C) {
        const float e = __expf(trans[i * C + j] - tmax);
        float v1 = G[i] * e;
        if constexpr (EC) v1 = __builtin_fmaf(N[i], e * ecost[i * C + j], v1);
        t1[i * C + j] = v1;
        t2[i * C + j] = N[i] * e;
      }
  }
}

// the parameter gradients from the per-sentence partials, sentences in the order of b, overwritten or accumulated:
// [dstart C | dend C | dtrans C*C | decost C*C] = sum_b grad[b] (cost-covariance part) + gz[b] (marginals part); decost has the
// edge marginals under grad and no gz part.
__global__ void path_param_reduce_kernel(const float* __restrict__ partial, const float* __restrict__ grad,
                                         const float* __restrict__ gz, int B, int C, float* __restrict__ dstart,
                                         float* __restrict__ dend, float* __restrict__ dtrans, float* __restrict__ decost,
                                         int accumulate) {
  const int cc = C * C, n = 4 * C + 2 * cc;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 2 * C + 2 * cc) return;
  int ia, ib;  // the partial under grad, the partial under gz (-1: none)
  float* d;
  if (i < 2 * C) {
    ia = i;
    ib = 2 * C + i;
    d = i < C ? dstart + i : dend + (i - C);
  } else if (i < 2 * C + cc) {
    ia = 4 * C + (i - 2 * C);
    ib = ia + cc;
    d = dtrans + (i - 2 * C);
  } else {
    if (!decost) return;
    ia = 4 * C + cc + (i - 2 * C - cc);
    ib = -1;
    d = decost + (i - 2 * C - cc);
  }
  float s = 0.f;
  if (gz && ib >= 0) {
    for (int b = 0; b < B; ++b) {
      s += grad[b] * partial[(long)b * n + ia];
      s += gz[b] * partial[(long)b * n + ib];
    }
  } else {
    for (int b = 0; b < B; ++b) s += grad[b] * partial[(long)b * n + ia];
  }
  if (accumulate) s += *d;
  *d = s;
}

// workspace, in floats, CT = 16, 32 or 64:  alpha [B,S,CT] | sp [B,S,CT] | ac [B,S,CT] | spf [B,S,CT] | mx [B,S] | mean [B,S] |
// partials [B, 4C + 2 C*C]
struct Ws {
  float *alpha, *sp, *ac, *spf, *mx, *mean, *partial;
};
inline size_t ws_floats(int B, int S, int C) {
  const size_t n = (size_t)B * S;
  return 4 * n * width(C) + 2 * n + (size_t)B * (4 * C + 2 * C * C);
}
inline Ws ws_of(void* p, int B, int S, int C) {
  const size_t n = (size_t)B * S;
  Ws w;
  w.alpha = (float*)p;
  w.sp = w.alpha + n * width(C);
  w.ac = w.sp + n * width(C);
  w.spf = w.ac + n * width(C);
  w.mx = w.spf + n * width(C);
  w.mean = w.mx + n;
  w.partial = w.mean + n;
  return w;
}

}  // namespace path
}  // namespace mtvaf

using namespace mtvaf;

extern "C" {

size_t mtvaf_crf_path_workspace_bytes(int B, int S, int C) {
  return bad_shape(B, S, C) ? 0 : path::ws_floats(B, S, C) * sizeof(float);
}

// risk [B] = the expected path cost; logz [B] nullable.  One launch; the workspace keeps what path_bwd reads.
int mtvaf_crf_path_fwd(const float* emissions, const float* cost, const float* ecost, const uint8_t* mask, const float* start,
                       const float* end, const float* trans, float* risk_out, float* logz, int B, int S, int C,
                       void* workspace, size_t workspace_bytes, hipStream_t st) {
  if (bad_shape(B, S, C)) return MTVAF_ERR_SHAPE;
  if (workspace_bytes < mtvaf_crf_path_workspace_bytes(B, S, C)) return MTVAF_ERR_WORKSPACE;
  const path::Ws w = path::ws_of(workspace, B, S, C);
#define PATH_FWD(CT, EC)                                                                                                 \
  hipLaunchKernelGGL((path::path_fwd_kernel<CT, EC>), dim3(B), dim3(64), 0, st, emissions, cost, ecost, mask, start, end, \
                     trans, w.alpha, w.sp, w.ac, w.spf, w.mx, w.mean, risk_out, logz, S, C)
#define PATH_FWD_W(CT)   \
  if (ecost)             \
    PATH_FWD(CT, true);  \
  else                   \
    PATH_FWD(CT, false)
  CRF_CHAIN_DISPATCH(C, PATH_FWD_W)
#undef PATH_FWD_W
#undef PATH_FWD
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

// gradients of sum_b grad[b] risk[b] + gz[b] logz[b] (gz nullable): demissions and dcost (nullable) with exact zeros at masked
// columns; dstart / dend / dtrans and decost (nullable) overwritten or accumulated.  cost and ecost must be those of the
// forward call that filled the workspace.  Two launches (the recursion, the reduction of the per-sentence partials).
int mtvaf_crf_path_bwd(const float* grad, const float* gz, const float* emissions, const float* cost, const float* ecost,
                       const uint8_t* mask, const float* start, const float* end, const float* trans, float* demissions,
                       float* dcost, float* decost, float* dstart, float* dend, float* dtrans, int accumulate, int B, int S,
                       int C, void* workspace, size_t workspace_bytes, hipStream_t st) {
  (void)start;  // (enters through the workspace's alphas)
  if (bad_shape(B, S, C)) return MTVAF_ERR_SHAPE;
  if (workspace_bytes < mtvaf_crf_path_workspace_bytes(B, S, C)) return MTVAF_ERR_WORKSPACE;
  const path::Ws w = path::ws_of(workspace, B, S, C);
#define PATH_BWD(CT, EC)                                                                                                  \
  hipLaunchKernelGGL((path::path_bwd_kernel<CT, EC>), dim3(B), dim3(64), 0, st, grad, gz, emissions, cost, ecost, mask, end, \
                     trans, w.alpha, w.sp, w.ac, w.spf, w.mx, w.mean, demissions, dcost, w.partial, S, C)
#define PATH_BWD_W(CT)   \
  if (ecost)             \
    PATH_BWD(CT, true);  \
  else                   \
    PATH_BWD(CT, false)
  CRF_CHAIN_DISPATCH(C, PATH_BWD_W)
#undef PATH_BWD_W
#undef PATH_BWD
  MTVAF_LAUNCH_CHECK();
  const int n = 2 * C + 2 * C * C;
  hipLaunchKernelGGL(path::path_param_reduce_kernel, dim3((n + 255) / 256), dim3(256), 0, st, w.partial, grad, gz, B, C, dstart,
                     dend, dtrans, decost, accumulate);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

}  // extern "C"
