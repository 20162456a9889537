// Linear-chain CRF: the EXPECTED COST (risk) of a column-additive cost under the chain's posterior, its gradients, and with
// them the vector-Jacobian product of the node marginals.  Extends the call sites of the reference's third-party CRF
// (models/bert_model.py:464 ctor, :521 likelihood), whose only trainable quantity is the log-likelihood.
//   cost fp32 [B,S,C];  R[b] = E_{y ~ p(.|x_b)} sum_{t < len_b} cost[b,t,y_t] = sum_t sum_c m_t(c) cost[b,t,c].
//   dR/dtheta = Cov_p(f_theta(y), cost(y)): beside the forward / backward variables it needs a second pair of recursions,
//     a_t(j) = E[cost of columns 0..t | y_t = j],  b_t(i) = E[cost of columns t+1.. | y_t = i]      (expectation semiring)
//     dR/dem[t,c] = m_t(c) (a_t(c) + b_t(c) - R),   dR/dtrans[i,j] = sum_{t>=1} xi_t(i,j) (a_{t-1}(i) + cost[t,j] + b_t(j) - R),
//     dR/dstart = dR/dem[0], dR/dend = dR/dem[len-1], dR/dcost[t,c] = m_t(c).
//   mask is a prefix mask; len_b = its leading ones; cost and emissions at or beyond len_b are never read.
// One wavefront per sentence, tag j on lane j, 1 <= C <= 64, 1 <= S <= 512; CT = 16, 32 or 64 is the unrolled width.  The
// scaled linear domain and the LDS lane broadcast are those of crf_wide.hip / crf_lattice.hip (the helpers are shared:
// crf_chain.h), and as in crf_lattice.hip two chains run interleaved in one wave through the same statements
// with the transition factors shared in registers: chain 0 is the scaled alpha (beta), chain 1 the cost-weighted one.
//
// CENTRING is part of the contract.  As written above a, b and R grow like len |cost| while every gradient is a difference
// of them, which in float32 loses len / |gradient| ulps.  Both recursions therefore subtract a per-step constant:
//     at_t(j) = cost[t,j] + sum_i w_t(i->j) ac_{t-1}(i),    ac_t = at_t - mean_t,   mean_t = sum_j p(y_t = j | x_0..t) at_t(j)
//     bc_{t-1}(i) = sum_j v_t(i->j) (cost[t,j] + bc_t(j)) - bmean_{t-1},   bmean_{t-1} = sum_j m_t(j) (cost[t,j] + bc_t(j))
// so ac, bc stay of the size of |cost| times the chain's correlation length.  A constant added to a_t or b_t cancels in
//     dR/dem[t,c] = m_t(c) (d_t(c) - dbar_t),   d_t = ac_t + bc_t,   dbar_t = sum_c m_t(c) d_t(c)
//     dR/dtrans   = sum_t xi_t(i,j) (ac_{t-1}(i) + cost[t,j] + bc_t(j) - dbar_t - mean_t)
// (the xi_t-weighted mean of the bracket's first three terms is dbar_t + mean_t: sum_i xi_t(i,j) (ac_{t-1}(i) + cost[t,j]) =
// m_t(j) at_t(j)), and R is summed on its own, in double: R = sum_t mean_t + sum_j p(y_{len-1} = j | x) ac_{len-1}(j).
// mean_t comes out of the broadcast that forms the next product (as the normaliser does) and bmean out of the same broadcast
// as the beta step, bit-identical in every lane: there is no cross-lane reduction on the serial path; dbar_t is a wave
// reduction off it.
//
// Exact zeros (none of them relies on the contraction mode, the file is compiled with the library's flags):
//   * cost identically zero on the live columns: at, mean, ac, bc, bmean, d, dbar are all +0.0 (sums and products of +0.0
//     with finite non-negative factors), so R == +0.0 and every gradient is +0.0 whatever the sign of g: dem and dcost are
//     written as g x + 0.0 and the parameter reduction starts its sum at +0.0, and (-0.0) + (+0.0) = +0.0;
//   * g[b] == 0: that sentence's dem, dcost and its share of dstart / dend / dtrans are g times a finite number, i.e. zeros,
//     written as +0.0 in the same way;
//   * masked columns of dem, dcost and marg are written as +0.0.
#include "crf_chain.h"

namespace mtvaf {
namespace risk {

constexpr int SMAX = CRF_CHAIN_SMAX;

// ---------------------------------------------------------------------------------------------
// forward.  s is the scaled alpha, u = s at the (signed) cost-weighted chain; both go through one broadcast, from which every
// lane takes   dot_t[j] = sum_i s_{t-1}[i] E[i][j],  sum = sum_i s_{t-1}[i],  dotu_t[j] = sum_i u_{t-1}[i] E[i][j],  sumu:
//     r = 1 / sum,  mean_{t-1} = sumu r,  sp_t = dot_t r,  s_t = sp_t x_t,   x_t[j] = exp(em_t[j] - mx_t),
//     at_t[j] = cost_t[j] + (dotu_t[j] / dot_t[j] - mean_{t-1})       (= cost_t + sum_i w_t(i->j) ac_{t-1}(i)).
// Left for the backward: alpha_ws[b][t] = s_t r_{t+1} (sum 1), sp_ws[b][t] = sp_t, ac_ws[b][t] = at_t - mean_t, mx_ws[b][t],
// mean_ws[b][t].  logZ as in crf_lattice.hip; R = sum_t mean_t + sum_j pe[j] ac_{len-1}[j] in double, pe the posterior of
// the last tag.
// ---------------------------------------------------------------------------------------------
template <int CT>
__global__ __launch_bounds__(64) void risk_fwd_kernel(const float* __restrict__ em, const float* __restrict__ cost,
                                                     const uint8_t* __restrict__ mask, const float* __restrict__ start,
                                                     const float* __restrict__ end, const float* __restrict__ trans,
                                                     float* __restrict__ alpha_ws, float* __restrict__ sp_ws,
                                                     float* __restrict__ ac_ws, float* __restrict__ mx_ws,
                                                     float* __restrict__ mean_ws, float* __restrict__ risk_out,
                                                     float* __restrict__ logz_out, int S, int C) {
  __shared__ __attribute__((aligned(16))) float bc[2][64];
  __shared__ float mxs[SMAX];
  __shared__ float rl[SMAX];
  __shared__ float mns[SMAX];
  const int b = blockIdx.x, j = threadIdx.x;
  const bool act = j < C, inct = j < CT;
  const int len = prefix_len(mask + (long)b * S, S, j);
  const float* emb = em + (long)b * S * C;
  const float* cb = cost + (long)b * S * C;
  for (int t = j; t < len; t += 64) {
    const float* e = emb + (long)t * C;
    float m = NEG;
    for (int i = 0; i < C; ++i) m = fmaxf(m, e[i]);
    mxs[t] = m;
    mx_ws[(long)b * S + t] = m;
  }
  __syncthreads();
  const float tmax = trans_max(trans, C, j);
  float w[CT];  // column j of E
#pragma unroll
  for (int i = 0; i < CT; ++i) w[i] = (act && i < C) ? __expf(trans[i * C + j] - tmax) : 0.f;
  const float a0 = act ? start[j] + emb[j] : NEG;
  const float c0 = wave_max(a0);
  float s = act ? __expf(a0 - c0) : 0.f;
  float at = act ? cb[j] : 0.f;
  float* al_p = alpha_ws + (long)b * S * CT + j;
  float* sp_p = sp_ws + (long)b * S * CT + j;
  float* ac_p = ac_ws + (long)b * S * CT + j;
  float en = (len > 1 && act) ? emb[C + j] : 0.f;
  float cn = (len > 1 && act) ? cb[C + j] : 0.f;
  for (int t = 1; t < len; ++t) {
    const float et = en, ct = cn;
    if (t + 1 < len && act) {
      en = emb[(long)(t + 1) * C + j];
      cn = cb[(long)(t + 1) * C + j];
    }
    bc[0][j] = s;
    bc[1][j] = s * at;
    lds_fence();
    float dot, sum, dotu, sumu;
    dot_sum<CT>(bc[0], w, dot, sum);
    dot_sum<CT>(bc[1], w, dotu, sumu);
    lds_fence();
    const float x = act ? __expf(et - mxs[t]) : 0.f;
    const float r = __builtin_amdgcn_rcpf(sum);
    const float mean = sumu * r;
    const float sp = dot * r;
    if (inct) {
      al_p[(long)(t - 1) * CT] = s * r;
      sp_p[(long)t * CT] = sp;
      ac_p[(long)(t - 1) * CT] = at - mean;
    }
    if (j == 0) {
      rl[t] = r;
      mns[t - 1] = mean;
    }
    at = (act && dot > 0.f) ? ct + (dotu * __builtin_amdgcn_rcpf(dot) - mean) : 0.f;
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
// backward, t = len-1 .. 1.  bt is the scaled beta of column t, bh = bc_t; u = x_t bt and q = u (cost_t + bh) go through one
// broadcast with sp_t, from which every lane i takes (row i of E)
//     eu = sum_j E[i][j] u[j],  d = sum_j sp_t[j] u[j],  eq = sum_j E[i][j] q[j],  dq = sum_j sp_t[j] q[j]:
//     ui_t = u / d,  mu_t = sp_t ui_t (node marginal),  beta_{t-1} = eu / d,  bmean_{t-1} = dq / d,  bc_{t-1} = eq / eu - bmean_{t-1},
//     xi_t[i][j] = alpha_ws[t-1][i] E[i][j] ui_t[j];  lane j accumulates column j of
//     G[i][j] = sum_t alpha_ws[t-1][i] ui_t[j] (ac_{t-1}[i] + k_t[j]),   k_t = cost_t + bc_t - dbar_t - mean_t.
//   MARG = false: dem[b,t,:] = g mu_t (d_t - dbar_t), dcost[b,t,:] = g mu_t (if asked), zeros at masked columns;
//                 partial[b] = [start C | end C | trans C*C] unweighted, weighted by g in risk_param_reduce_kernel.
//   MARG = true:  the beta chain alone, dem = mu itself (the marginals of risk_fwd).
// ---------------------------------------------------------------------------------------------
template <int CT, bool MARG>
__global__ __launch_bounds__(64) void risk_bwd_kernel(const float* __restrict__ grad, const float* __restrict__ em,
                                                     const float* __restrict__ cost, const uint8_t* __restrict__ mask,
                                                     const float* __restrict__ end, const float* __restrict__ trans,
                                                     const float* __restrict__ alpha_ws, const float* __restrict__ sp_ws,
                                                     const float* __restrict__ ac_ws, const float* __restrict__ mx_ws,
                                                     const float* __restrict__ mean_ws, float* __restrict__ dem,
                                                     float* __restrict__ dcost, float* __restrict__ partial, int S, int C) {
  __shared__ __attribute__((aligned(16))) float bu[64];
  __shared__ __attribute__((aligned(16))) float bs[64];
  __shared__ __attribute__((aligned(16))) float bq[64];
  __shared__ __attribute__((aligned(16))) float ba[64];
  __shared__ __attribute__((aligned(16))) float bp[64];
  __shared__ float mxs[SMAX];
  __shared__ float mns[SMAX];
  const int b = blockIdx.x, j = threadIdx.x;
  const bool act = j < C, inct = j < CT;
  const int len = prefix_len(mask + (long)b * S, S, j);
  const float* emb = em + (long)b * S * C;
  const float* cb = MARG ? nullptr : cost + (long)b * S * C;
  for (int t = j; t < len; t += 64) {
    mxs[t] = mx_ws[(long)b * S + t];
    if constexpr (!MARG) mns[t] = mean_ws[(long)b * S + t];
  }
  __syncthreads();
  const float tmax = trans_max(trans, C, j);
  float wr[CT];  // row j of E
#pragma unroll
  for (int i = 0; i < CT; ++i) wr[i] = (act && i < C) ? __expf(trans[j * C + i] - tmax) : 0.f;
  const float g = MARG ? 1.f : grad[b];
  float G[MARG ? 1 : CT];
  if constexpr (!MARG) {
#pragma unroll
    for (int i = 0; i < CT; ++i) G[i] = 0.f;
  }
  const float* al_p = alpha_ws + (long)b * S * CT + j;
  const float* sp_p = sp_ws + (long)b * S * CT + j;
  const float* ac_p = ac_ws + (long)b * S * CT + j;
  const float em_ = wave_max(act ? end[j] : NEG);
  float bt = act ? __expf(end[j] - em_) : 0.f;  // beta of the last column, any positive scale
  float bh = 0.f;                               // bc of the last column
  float* ob = dem + (long)b * S * C;
  float* oc = (!MARG && dcost) ? dcost + (long)b * S * C : nullptr;
  float acur = (!MARG && inct) ? ac_p[(long)(len - 1) * CT] : 0.f;  // ac of the column being written
  float dend_v = 0.f;
  float en = (len > 1 && act) ? emb[(long)(len - 1) * C + j] : 0.f;
  float cn = (!MARG && len > 1 && act) ? cb[(long)(len - 1) * C + j] : 0.f;
  float spn = (len > 1 && inct) ? sp_p[(long)(len - 1) * CT] : 0.f;
  float aln = (!MARG && len > 1 && inct) ? al_p[(long)(len - 2) * CT] : 0.f;
  float acn = (!MARG && len > 1 && inct) ? ac_p[(long)(len - 2) * CT] : 0.f;
  for (int t = len - 1; t >= 1; --t) {
    const float et = en, ct = cn, spv = spn, alv = aln, acv = acn;
    if (t >= 2) {
      if (act) {
        en = emb[(long)(t - 1) * C + j];
        if constexpr (!MARG) cn = cb[(long)(t - 1) * C + j];
      }
      if (inct) {
        spn = sp_p[(long)(t - 1) * CT];
        if constexpr (!MARG) {
          aln = al_p[(long)(t - 2) * CT];
          acn = ac_p[(long)(t - 2) * CT];
        }
      }
    }
    const float x = act ? __expf(et - mxs[t]) : 0.f;
    const float u = x * bt;
    bu[j] = u;
    bs[j] = spv;
    if constexpr (!MARG) {
      bq[j] = u * (ct + bh);
      ba[j] = alv;
      bp[j] = alv * acv;
    }
    lds_fence();
    float eu, d;
    dot_dot<CT>(bu, bs, wr, eu, d);
    const float r = __builtin_amdgcn_rcpf(d);
    const float ui = u * r;
    const float mu = spv * ui;
    bt = eu * r;
    if constexpr (MARG) {
      lds_fence();
      if (act) ob[(long)t * C + j] = mu;
    } else {
      float eq, dq;
      dot_dot<CT>(bq, bs, wr, eq, dq);
      const float dv = acur + bh;
      const float dbar = wave_sum(mu * dv);
      const float val = mu * (dv - dbar);
      const float k = ui * (((ct + bh) - dbar) - mns[t]);
      const f4* a4 = reinterpret_cast<const f4*>(ba);
      const f4* p4 = reinterpret_cast<const f4*>(bp);
#pragma unroll
      for (int q = 0; q < CT / 4; ++q) {
        const f4 a = a4[q], p = p4[q];
        G[4 * q] = __builtin_fmaf(a.x, k, __builtin_fmaf(p.x, ui, G[4 * q]));
        G[4 * q + 1] = __builtin_fmaf(a.y, k, __builtin_fmaf(p.y, ui, G[4 * q + 1]));
        G[4 * q + 2] = __builtin_fmaf(a.z, k, __builtin_fmaf(p.z, ui, G[4 * q + 2]));
        G[4 * q + 3] = __builtin_fmaf(a.w, k, __builtin_fmaf(p.w, ui, G[4 * q + 3]));
      }
      lds_fence();
      bh = (act && eu > 0.f) ? eq * __builtin_amdgcn_rcpf(eu) - dq * r : 0.f;
      if (t == len - 1) dend_v = val;
      acur = acv;
      if (act) {
        ob[(long)t * C + j] = g * val + 0.f;  // (+ 0.f: a zero product is written as +0.0 whatever the signs)
        if (oc) oc[(long)t * C + j] = g * mu + 0.f;
      }
    }
  }
  const float p0 = (inct ? al_p[0] : 0.f) * bt;
  const float p0n = p0 * __builtin_amdgcn_rcpf(wave_sum(p0));
  if constexpr (MARG) {
    if (act) ob[j] = p0n;
    for (int idx = len * C + j; idx < S * C; idx += 64) ob[idx] = 0.f;  // masked columns: exact zeros
  } else {
    const float dv = acur + bh;
    const float dbar = wave_sum(p0n * dv);
    const float val = p0n * (dv - dbar);
    if (len == 1) dend_v = val;
    if (act) {
      ob[j] = g * val + 0.f;
      if (oc) oc[j] = g * p0n + 0.f;
    }
    for (int idx = len * C + j; idx < S * C; idx += 64) {  // masked columns: exact zeros
      ob[idx] = 0.f;
      if (oc) oc[idx] = 0.f;
    }
    if (act) {
      float* pp = partial + (long)b * (2 * C + C * C);
      pp[j] = val;
      pp[C + j] = dend_v;
#pragma unroll
      for (int i = 0; i < CT; ++i)
        if (i < C) pp[2 * C + i * C + j] = G[i] * __expf(trans[i * C + j] - tmax);
    }
  }
}

// d[i] = sum_b grad[b] partial[b][i] in the order of b, overwritten or accumulated (crf_chain.h; compiled here with the
// library's contraction mode, so not the same instructions as crf_lattice.hip's reduction)
__global__ void risk_param_reduce_kernel(const float* __restrict__ partial, const float* __restrict__ grad, int B, int C,
                                         float* __restrict__ dstart, float* __restrict__ dend, float* __restrict__ dtrans,
                                         int accumulate) {
  param_reduce(partial, grad, B, C, dstart, dend, dtrans, accumulate);
}

// workspace, in floats, CT = 16, 32 or 64:  alpha [B,S,CT] | sp [B,S,CT] | ac [B,S,CT] | mx [B,S] | mean [B,S] |
// partials [B, 2C + C*C]
struct Ws {
  float *alpha, *sp, *ac, *mx, *mean, *partial;
};
inline size_t ws_floats(int B, int S, int C) {
  const size_t n = (size_t)B * S;
  return 3 * n * width(C) + 2 * n + (size_t)B * (2 * C + C * C);
}
inline Ws ws_of(void* p, int B, int S, int C) {
  const size_t n = (size_t)B * S;
  Ws w;
  w.alpha = (float*)p;
  w.sp = w.alpha + n * width(C);
  w.ac = w.sp + n * width(C);
  w.mx = w.ac + n * width(C);
  w.mean = w.mx + n;
  w.partial = w.mean + n;
  return w;
}

template <bool MARG>
int launch_bwd(const float* grad, const float* em, const float* cost, const uint8_t* mask, const float* end,
               const float* trans, const Ws& w, float* dem, float* dcost, int B, int S, int C, hipStream_t st) {
#define RISK_BWD(CT)                                                                                                  \
  hipLaunchKernelGGL((risk_bwd_kernel<CT, MARG>), dim3(B), dim3(64), 0, st, grad, em, cost, mask, end, trans, w.alpha, \
                     w.sp, w.ac, w.mx, w.mean, dem, dcost, w.partial, S, C)
  CRF_CHAIN_DISPATCH(C, RISK_BWD)
#undef RISK_BWD
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

}  // namespace risk
}  // namespace mtvaf

using namespace mtvaf;

extern "C" {

size_t mtvaf_crf_risk_workspace_bytes(int B, int S, int C) {
  return bad_shape(B, S, C) ? 0 : risk::ws_floats(B, S, C) * sizeof(float);
}

// risk [B] = the expected cost; logz [B] and marg [B,S,C] nullable.  One launch (two with marg: the beta chain alone); the
// workspace keeps what risk_bwd reads.
int mtvaf_crf_risk_fwd(const float* emissions, const float* cost, const uint8_t* mask, const float* start, const float* end,
                       const float* trans, float* risk_out, float* logz, float* marg, int B, int S, int C, void* workspace,
                       size_t workspace_bytes, hipStream_t st) {
  if (bad_shape(B, S, C)) return MTVAF_ERR_SHAPE;
  if (workspace_bytes < mtvaf_crf_risk_workspace_bytes(B, S, C)) return MTVAF_ERR_WORKSPACE;
  const risk::Ws w = risk::ws_of(workspace, B, S, C);
#define RISK_FWD(CT)                                                                                                   \
  hipLaunchKernelGGL(risk::risk_fwd_kernel<CT>, dim3(B), dim3(64), 0, st, emissions, cost, mask, start, end, trans, w.alpha, \
                     w.sp, w.ac, w.mx, w.mean, risk_out, logz, S, C)
  CRF_CHAIN_DISPATCH(C, RISK_FWD)
#undef RISK_FWD
  MTVAF_LAUNCH_CHECK();
  if (!marg) return MTVAF_OK;
  return risk::launch_bwd<true>(nullptr, emissions, nullptr, mask, end, trans, w, marg, nullptr, B, S, C, st);
}

// gradients of sum_b grad[b] risk[b]: demissions and dcost (nullable) with exact zeros at masked columns; the parameter
// gradients overwritten or accumulated.  Two launches (the recursion, the reduction of the per-sentence partials).
int mtvaf_crf_risk_bwd(const float* grad, const float* emissions, const float* cost, const uint8_t* mask, const float* start,
                       const float* end, const float* trans, float* demissions, float* dcost, float* dstart, float* dend,
                       float* dtrans, int accumulate, int B, int S, int C, void* workspace, size_t workspace_bytes,
                       hipStream_t st) {
  (void)start;  // (enters through the workspace's alphas)
  if (bad_shape(B, S, C)) return MTVAF_ERR_SHAPE;
  if (workspace_bytes < mtvaf_crf_risk_workspace_bytes(B, S, C)) return MTVAF_ERR_WORKSPACE;
  const risk::Ws w = risk::ws_of(workspace, B, S, C);
  if (int rc = risk::launch_bwd<false>(grad, emissions, cost, mask, end, trans, w, demissions, dcost, B, S, C, st)) return rc;
  const int n = 2 * C + C * C;
  hipLaunchKernelGGL(risk::risk_param_reduce_kernel, dim3((n + 255) / 256), dim3(256), 0, st, w.partial, grad, B, C, dstart,
                     dend, dtrans, accumulate);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

}  // extern "C"
