// Linear-chain CRF for wide tag sets, 16 < C <= 64 (crf.hip keeps C <= 16).  Same contracts as crf.hip's K12 / K13
// kernels: masked NLL forward (gold-path score - logZ), its analytic backward, masked Viterbi with the lowest index
// winning ties.
// One wavefront per sentence, tag j on lane j; lanes j >= C are neutral (0 in the scaled linear domain, -1e30 in
// max-plus).  The recursions run in crf.hip's scaled linear domain (no exp / log on the serial path).  The C-term
// product of a step is a lane broadcast through LDS: every lane writes its value, reads the CT values back with
// CT/4 broadcast ds_read_b128 and multiplies them against a column (or row) of the transition matrix held in CT
// registers, CT = C rounded up to 16 (32, 48 or 64).  Per step, forward, at CT = 64: 1 ds_write + 16 ds_read_b128
// + 32 v_pk_fma_f32 + the 4-DPP-add row sums and 4 v_readlane of the normaliser + ~8 VALU + 2 global stores.
// Per-step operands (emission rows, predicted alphas) are fetched CHUNK steps ahead into registers; nothing is held
// per time step in LDS except mask, tags, maxima and the Viterbi back-pointers (one byte per step and tag), so no
// kernel needs more than the default 64 KiB and nothing is set on a function at launch.
#include "crf_chain.h"
#include "crf_wide.h"

namespace mtvaf {
namespace crfw {

constexpr int CHUNK = 16;  // steps whose per-step operands are loaded together, one chunk ahead of use

template <int K>
__device__ __forceinline__ float ror16(float v) {  // DPP row_ror:K
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x120 + K, 0xf, 0xf, true));
}

// sum over the first CT lanes, wave-uniform and bit-identical everywhere: row sums by DPP rotation, then the row
// results added in a fixed order
template <int CT>
__device__ __forceinline__ float sum_u(float v) {
  v += ror16<8>(v);
  v += ror16<4>(v);
  v += ror16<2>(v);
  v += ror16<1>(v);
  float s = lane_val(v, 0) + lane_val(v, 16);
  if (CT > 32) s += lane_val(v, 32);
  if (CT > 48) s += lane_val(v, 48);
  return s;
}

// this lane's value to LDS, then sum_i bc[i] * w[i] over the CT broadcast values (lds_fence: the reads stay behind the write).
// The products are v_pk_fma_f32 on register pairs as the broadcast reads deliver them (w holds pairs (i, i+1)).
template <int CT>
__device__ __forceinline__ float bcast_dot(float* bc, int lane, float v, const f32x2 (&w)[CT / 2]) {
  bc[lane] = v;
  lds_fence();
  const f4* b4 = reinterpret_cast<const f4*>(bc);
  f32x2 a0 = {0.f, 0.f}, a1 = {0.f, 0.f};
#pragma unroll
  for (int q = 0; q < CT / 4; ++q) {
    const f4 x = b4[q];
    a0 = __builtin_elementwise_fma(f32x2{x.x, x.y}, w[2 * q], a0);
    a1 = __builtin_elementwise_fma(f32x2{x.z, x.w}, w[2 * q + 1], a1);
  }
  return (a0.x + a0.y) + (a1.x + a1.y);
}

// the lane-strided staging every kernel starts with: mask, and optionally tags and per-step emission maxima
__device__ __forceinline__ void stage(const float* __restrict__ em, const int64_t* __restrict__ tags,
                                      const uint8_t* __restrict__ mask, long b, int S, int C, int lane, uint8_t* mk,
                                      int* tg, float* mxs, float* mx_out) {
  for (int t = lane; t < S; t += 64) {
    mk[t] = mask[b * S + t];
    if (tg) tg[t] = (int)tags[b * S + t];
    if (mxs) {
      const float* e = em + (b * S + t) * C;
      float m = NEG;
      for (int i = 0; i < C; ++i) m = fmaxf(m, e[i]);
      mxs[t] = m;
      if (mx_out) mx_out[b * S + t] = m;
    }
  }
}

__device__ __forceinline__ int mask_count(const uint8_t* mk, int S, int lane) {
  int cnt = 0;
  for (int t = lane; t < S; t += 64) cnt += mk[t] ? 1 : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  return cnt;
}

// ---------------------------------------------------------------------------------------------
// forward.  s is the scaled alpha, r = 1 / sum(s) is applied one step late so that its reduction runs beside the
// next product instead of in front of it:
//     dot_t[j] = sum_i s_{t-1}[i] E[i][j],   s_t[j] = dot_t[j] x_t[j] r_{t-1},   log K_t = log K_{t-1} + tmax + mx_t - log r
// with alpha_t = K_t s_t.  alpha_ws[t] = s_t (every t; carried over masked steps), sp_ws[t] = dot_t (the predicted
// alpha the backward needs, on the same scale as alpha_ws[t-1]), mx_ws[t] = max_j emit_t[j].
// GOLD = false (tag marginals): no tags are read, no gold-path score is formed, llh is not written.
// ---------------------------------------------------------------------------------------------
template <int CT, bool GOLD>
__global__ __launch_bounds__(64) void crf_wide_fwd_kernel(const float* __restrict__ em, const int64_t* __restrict__ tags,
                                                         const uint8_t* __restrict__ mask, const float* __restrict__ start,
                                                         const float* __restrict__ end, const float* __restrict__ trans,
                                                         float* __restrict__ alpha_ws, float* __restrict__ sp_ws,
                                                         float* __restrict__ mx_ws, float* __restrict__ logz,
                                                         float* __restrict__ llh, int S, int C) {
  __shared__ __attribute__((aligned(16))) float bc[64];
  extern __shared__ __attribute__((aligned(16))) float crfw_lds[];
  float* mxs = crfw_lds;                              // [S] emission maxima
  float* rl = mxs + S;                                // [S] r applied at step t
  int* tg = reinterpret_cast<int*>(rl + S);           // [S]
  uint8_t* mk = reinterpret_cast<uint8_t*>(tg + S);   // [S]
  const int b = blockIdx.x, j = threadIdx.x;
  const bool act = j < C;
  const float* emb = em + (long)b * S * C;
  stage(em, tags, mask, b, S, C, j, mk, GOLD ? tg : nullptr, mxs, mx_ws);
  const float tmax = trans_max(trans, C, j);
  f32x2 w[CT / 2];  // column j of E = exp(trans - tmax), rows (2p, 2p+1) in w[p]
#pragma unroll
  for (int i = 0; i < CT; ++i) w[i / 2][i % 2] = (act && i < C) ? __expf(trans[i * C + j] - tmax) : 0.f;
  const float a0l = act ? start[j] + emb[j] : NEG;
  const float c0 = wave_max(a0l);
  float s = act ? __expf(a0l - c0) : 0.f;
  float* aw = alpha_ws + (long)b * S * CT + j;
  float* pw = sp_ws + (long)b * S * CT + j;
  if (j < CT) aw[0] = s;
  float r = __builtin_amdgcn_rcpf(sum_u<CT>(s));
  __syncthreads();
  const float* er = emb + j;
  float ec[CHUNK], en[CHUNK];
#pragma unroll
  for (int q = 0; q < CHUNK; ++q) ec[q] = (act && q < S) ? er[(long)q * C] : 0.f;
  for (int t0 = 0; t0 < S; t0 += CHUNK) {
#pragma unroll
    for (int q = 0; q < CHUNK; ++q) {
      const int t = t0 + CHUNK + q;
      en[q] = (act && t < S) ? er[(long)t * C] : 0.f;
    }
    const int tq = t0 + (j & (CHUNK - 1));
    const bool onq = j < CHUNK && tq >= 1 && tq < S && mk[tq] != 0;
    const unsigned long long mb = __ballot(onq);
    const float mxq = tq < S ? mxs[tq] : 0.f;
    const int nq = min(CHUNK, S - t0);
#pragma unroll
    for (int q = 0; q < CHUNK; ++q) {
      if (q < nq) {
        const int t = t0 + q;
        if ((mb >> q) & 1) {  // (wave-uniform)
          const float xr = (act ? __expf(ec[q] - lane_val(mxq, q)) : 0.f) * r;
          const float dot = bcast_dot<CT>(bc, j, s, w);
          if (j < CT) pw[(long)t * CT] = dot;
          rl[t] = r;
          s = dot * xr;
          r = __builtin_amdgcn_rcpf(sum_u<CT>(s));
        }
        if (j < CT) aw[(long)t * CT] = s;
      }
    }
#pragma unroll
    for (int q = 0; q < CHUNK; ++q) ec[q] = en[q];
  }
  const float em_ = wave_max(act ? end[j] : NEG);
  const float fin = wave_sum(act ? s * __expf(end[j] - em_) : 0.f);
  __syncthreads();
  float lz = 0.f, sc = 0.f;
  int cnt = 0;
  for (int t = j; t < S; t += 64) {
    cnt += mk[t] ? 1 : 0;
    if (t >= 1 && mk[t]) {
      lz += mxs[t] + tmax - __logf(rl[t]);
      if constexpr (GOLD) sc += trans[tg[t - 1] * C + tg[t]] + emb[(long)t * C + tg[t]];
    }
  }
  lz = wave_sum(lz);
  if constexpr (GOLD) {
    sc = wave_sum(sc);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  }
  if (j == 0) {
    const float z = c0 + lz + __logf(fin) + em_;
    if constexpr (GOLD) sc += start[tg[0]] + emb[tg[0]] + end[tg[max(cnt - 1, 0)]];
    logz[b] = z;
    if constexpr (GOLD) llh[b] = sc - z;
  }
}

// ---------------------------------------------------------------------------------------------
// backward, as crf.hip's: b_t scaled so that the node marginals need no normaliser beyond one sum per step.
//   serial, t = S-1 .. 1:  u = x_t b_t,  d = sp_t . u,  ui_t = u / d,  node marginal sp_t ui_t,  b_{t-1} = (E u) / d
//   (lane j holds row j of E; d's reduction runs beside the broadcast product).  d(emissions) leave per step, ui_t
//   goes to the workspace; then the summed edge marginals sum_t a_{t-1}[i] ui_t[j] = (A^T UI)[i][j] run on the matrix
//   cores, 16 time steps at a time, the next block's operands loaded while the current one multiplies.
// partial layout per sequence: [start C | end C | trans C*C] (crf.hip's crf_param_reduce_kernel sums them).
// GRAD (crf_wide.h): CRF_GRAD_MEAN scales by *gout / B; CRF_GRAD_SENTENCE by -gout[b] (d(emissions) of sum_b gout[b] llh[b];
// the partials take their weight in the reduction); CRF_MARGINALS writes the node marginals to dem and ends after the
// serial part: no tags, no gold counts, no ui rows, no edge-marginal product, no partials.
// ---------------------------------------------------------------------------------------------
template <int CT, int GRAD>
__global__ __launch_bounds__(64) void crf_wide_bwd_kernel(const float* __restrict__ em, const int64_t* __restrict__ tags,
                                                         const uint8_t* __restrict__ mask, const float* __restrict__ end,
                                                         const float* __restrict__ trans, const float* __restrict__ alpha_ws,
                                                         const float* __restrict__ sp_ws, const float* __restrict__ mx_ws,
                                                         float* __restrict__ ui_ws, const float* __restrict__ gout,
                                                         float* __restrict__ dem, float* __restrict__ partial, int B, int S,
                                                         int C) {
  __shared__ __attribute__((aligned(16))) float bc[64];
  constexpr bool MARG = GRAD == CRF_MARGINALS;
  __shared__ float gold[MARG ? 1 : CT * CT];  // gold transition counts
  extern __shared__ __attribute__((aligned(16))) float crfw_lds[];
  float* mxs = crfw_lds;                              // [S]
  int* tg = reinterpret_cast<int*>(mxs + S);          // [S]
  uint8_t* mk = reinterpret_cast<uint8_t*>(tg + S);   // [S]
  const int b = blockIdx.x, j = threadIdx.x;
  const bool act = j < C;
  const float* emb = em + (long)b * S * C;
  stage(em, tags, mask, b, S, C, j, mk, MARG ? nullptr : tg, nullptr, nullptr);
  for (int t = j; t < S; t += 64) mxs[t] = mx_ws[(long)b * S + t];
  if constexpr (!MARG)
    for (int i = j; i < CT * CT; i += 64) gold[i] = 0.f;
  __syncthreads();
  if constexpr (!MARG)
    for (int t = 1 + j; t < S; t += 64)
      if (mk[t]) atomicAdd(&gold[tg[t - 1] * CT + tg[t]], 1.f);  // (integer-valued sums: exact, order-independent)
  // (marginal - one-hot) below is d(-llh): the per-sentence weight enters negated
  const float g = MARG ? 1.f : (GRAD == CRF_GRAD_SENTENCE ? -gout[b] : (gout ? *gout : 1.f) / B);
  const float tmax = trans_max(trans, C, j);
  f32x2 wr[CT / 2];  // row j of E, columns (2p, 2p+1) in wr[p]
#pragma unroll
  for (int i = 0; i < CT; ++i) wr[i / 2][i % 2] = (act && i < C) ? __expf(trans[j * C + i] - tmax) : 0.f;
  const int cnt = MARG ? 0 : mask_count(mk, S, j);
  const int last_tag = MARG ? 0 : tg[max(cnt - 1, 0)];
  const float* alb = alpha_ws + (long)b * S * CT;
  const float* spb = sp_ws + (long)b * S * CT;
  float* uib = ui_ws + (long)b * S * CT;
  float* deb = dem + (long)b * S * C;
  const float em_ = wave_max(act ? end[j] : NEG);
  float bt = act ? __expf(end[j] - em_) : 0.f;  // beta of the last position, any positive scale
  float dend = 0.f;
  if constexpr (!MARG) {
    const float pe = act ? alb[(long)(S - 1) * CT + j] * bt : 0.f;
    dend = pe * __frcp_rn(wave_sum(pe)) - (j == last_tag ? 1.f : 0.f);
  }
  __syncthreads();
  {
    const float* er = emb + j;
    const float* sr = spb + j;
    float ec[CHUNK], sc[CHUNK], en[CHUNK], sn[CHUNK];
#pragma unroll
    for (int q = 0; q < CHUNK; ++q) {
      const int t = S - 1 - q;
      ec[q] = (act && t >= 1) ? er[(long)t * C] : 0.f;
      sc[q] = (act && t >= 1) ? sr[(long)t * CT] : 0.f;
    }
    for (int hi = S - 1; hi >= 1; hi -= CHUNK) {  // steps hi, hi-1, .., max(hi - CHUNK + 1, 1)
#pragma unroll
      for (int q = 0; q < CHUNK; ++q) {
        const int t = hi - CHUNK - q;
        en[q] = (act && t >= 1) ? er[(long)t * C] : 0.f;
        sn[q] = (act && t >= 1) ? sr[(long)t * CT] : 0.f;
      }
      const int tq = hi - (j & (CHUNK - 1));
      const bool onq = j < CHUNK && tq >= 1 && mk[tq] != 0;
      const unsigned long long mb = __ballot(onq);
      const float mxq = tq >= 1 ? mxs[tq] : 0.f;
      const int tgq = (!MARG && tq >= 1) ? tg[tq] : -1;
      const int nq = min(CHUNK, hi);
#pragma unroll
      for (int q = 0; q < CHUNK; ++q) {
        if (q < nq) {
          const int t = hi - q;
          float ui = 0.f, de = 0.f;
          if ((mb >> q) & 1) {  // (wave-uniform)
            const float x = act ? __expf(ec[q] - lane_val(mxq, q)) : 0.f;
            const float u = x * bt;
            const float rd = __builtin_amdgcn_rcpf(sum_u<CT>(sc[q] * u));
            const float dot = bcast_dot<CT>(bc, j, u, wr);
            ui = u * rd;
            if constexpr (MARG) de = sc[q] * ui;
            else de = g * (sc[q] * ui - (j == lane_val(tgq, q) ? 1.f : 0.f));
            bt = dot * rd;
          }
          if constexpr (!MARG)
            if (j < CT) uib[(long)t * CT + j] = ui;
          if (act) deb[(long)t * C + j] = de;
        }
      }
#pragma unroll
      for (int q = 0; q < CHUNK; ++q) {
        ec[q] = en[q];
        sc[q] = sn[q];
      }
    }
  }
  {
    const float p0 = act ? alb[j] * bt : 0.f;
    const float p0n = p0 * __frcp_rn(wave_sum(p0));
    if constexpr (MARG) {
      if (act) deb[j] = p0n;
      return;
    }
    float* pp = partial + (long)b * (2 * C + C * C);
    if (act) {
      const float oh = j == tg[0] ? 1.f : 0.f;
      deb[j] = g * (p0n - oh);
      pp[j] = p0n - oh;
      pp[C + j] = dend;
    }
  }
  __syncthreads();  // ui_ws written above is read back below by other lanes
  // G[i][j] = sum_{t >= 1} a_{t-1}[i] ui_t[j]: A[m = i][k = t] = alpha row t-1, B[k = t][n = j] = ui row t;
  // 16 x 16 tiles (ti, tj), 4 time steps per v_mfma_f32_16x16x4f32, 16 per block
  constexpr int T = CT / 16;
  const int m = j & 15, k4 = j >> 4;
  f4 acc[T][T];
#pragma unroll
  for (int ti = 0; ti < T; ++ti)
#pragma unroll
    for (int tj = 0; tj < T; ++tj) acc[ti][tj] = f4{0.f, 0.f, 0.f, 0.f};
  float av[4][T], uv[4][T], an[4][T], un[4][T];
  auto load_block = [&](int t0, float (&a)[4][T], float (&u)[4][T]) {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int t = t0 + 4 * kk + k4;
#pragma unroll
      for (int ti = 0; ti < T; ++ti) {
        a[kk][ti] = t < S ? alb[(long)(t - 1) * CT + 16 * ti + m] : 0.f;
        u[kk][ti] = t < S ? uib[(long)t * CT + 16 * ti + m] : 0.f;
      }
    }
  };
  load_block(1, av, uv);
  for (int t0 = 1; t0 < S; t0 += 16) {
    load_block(t0 + 16, an, un);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
      for (int ti = 0; ti < T; ++ti)
#pragma unroll
        for (int tj = 0; tj < T; ++tj)
          acc[ti][tj] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[kk][ti], uv[kk][tj], acc[ti][tj], 0, 0, 0);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
      for (int ti = 0; ti < T; ++ti) {
        av[kk][ti] = an[kk][ti];
        uv[kk][ti] = un[kk][ti];
      }
  }
  float* pp = partial + (long)b * (2 * C + C * C) + 2 * C;
#pragma unroll
  for (int ti = 0; ti < T; ++ti)
#pragma unroll
    for (int tj = 0; tj < T; ++tj)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 16 * ti + 4 * k4 + r, jj = 16 * tj + m;
        if (i < C && jj < C) pp[i * C + jj] = acc[ti][tj][r] * __expf(trans[i * C + jj] - tmax) - gold[i * CT + jj];
      }
}

// ---------------------------------------------------------------------------------------------
// Viterbi: lane j keeps column j of the transitions; best = max_i (score[i] + trans[i][j]) over the broadcast scores,
// scanned in 4 interleaved chains (ascending i, strict >, so each keeps its lowest index) merged with the lowest index
// winning ties, as torch.max.  Back-pointers are one byte per (step, tag), four steps per word; the backtrace reads
// lane `cur` of a word with one v_readlane per step.
// ---------------------------------------------------------------------------------------------
template <int CT>
__device__ __forceinline__ void vit_best(float* bc, int lane, float score, const float (&tc)[CT], float& best, int& bi) {
  bc[lane] = score;
  lds_fence();
  const f4* b4 = reinterpret_cast<const f4*>(bc);
  float bv[4] = {NEG, NEG, NEG, NEG};
  int bx[4] = {0, 1, 2, 3};
#pragma unroll
  for (int q = 0; q < CT / 4; ++q) {
    const f4 x = b4[q];
    const float v[4] = {x.x + tc[4 * q], x.y + tc[4 * q + 1], x.z + tc[4 * q + 2], x.w + tc[4 * q + 3]};
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (q == 0 || v[c] > bv[c]) {
        bv[c] = v[c];
        bx[c] = 4 * q + c;
      }
  }
#pragma unroll
  for (int c = 1; c < 4; ++c)
    if (bv[c] > bv[0] || (bv[c] == bv[0] && bx[c] < bx[0])) {
      bv[0] = bv[c];
      bx[0] = bx[c];
    }
  best = bv[0];
  bi = bx[0];
}

template <int CT>
__global__ __launch_bounds__(64) void crf_wide_viterbi_kernel(const float* __restrict__ em, const uint8_t* __restrict__ mask,
                                                             const float* __restrict__ start, const float* __restrict__ end,
                                                             const float* __restrict__ trans, int32_t* __restrict__ tags_out,
                                                             int32_t* __restrict__ lens_out, int S, int C) {
  __shared__ __attribute__((aligned(16))) float bc[64];
  extern __shared__ __attribute__((aligned(16))) float crfw_lds[];
  const int S4 = (S + 3) >> 2;
  uint32_t* bpw = reinterpret_cast<uint32_t*>(crfw_lds);   // [S4][64] back-pointers, byte t & 3 of word t >> 2
  int* path = reinterpret_cast<int*>(bpw + S4 * 64);       // [S]
  uint8_t* mk = reinterpret_cast<uint8_t*>(path + S);      // [S]
  const int b = blockIdx.x, j = threadIdx.x;
  const bool act = j < C;
  const float* emb = em + (long)b * S * C;
  stage(em, nullptr, mask, b, S, C, j, mk, nullptr, nullptr, nullptr);
  float tc[CT];  // column j of the transitions; NEG for padding candidates (never win) and in lanes beyond C
#pragma unroll
  for (int i = 0; i < CT; ++i) tc[i] = (act && i < C) ? trans[i * C + j] : NEG;
  float score = act ? start[j] + emb[j] : NEG;
  __syncthreads();
  const int cnt = mask_count(mk, S, j);
  const float* er = emb + j;
  float ec[CHUNK], en[CHUNK];
#pragma unroll
  for (int q = 0; q < CHUNK; ++q) ec[q] = (act && q < S) ? er[(long)q * C] : 0.f;
  uint32_t wb = 0;
  for (int t0 = 0; t0 < S; t0 += CHUNK) {
#pragma unroll
    for (int q = 0; q < CHUNK; ++q) {
      const int t = t0 + CHUNK + q;
      en[q] = (act && t < S) ? er[(long)t * C] : 0.f;
    }
    const int tq = t0 + (j & (CHUNK - 1));
    const bool onq = j < CHUNK && tq >= 1 && tq < S && mk[tq] != 0;
    const unsigned long long mb = __ballot(onq);
    const int nq = min(CHUNK, S - t0);
#pragma unroll
    for (int q = 0; q < CHUNK; ++q) {
      const int t = t0 + q;
      if (q < nq && t >= 1) {
        float best;
        int bi;
        vit_best<CT>(bc, j, score, tc, best, bi);
        wb |= (uint32_t)bi << (8 * (q & 3));
        if ((mb >> q) & 1) score = act ? best + ec[q] : NEG;  // (wave-uniform)
        if ((q & 3) == 3 || t == S - 1) {
          bpw[(t >> 2) * 64 + j] = wb;
          wb = 0;
        }
      }
    }
#pragma unroll
    for (int q = 0; q < CHUNK; ++q) ec[q] = en[q];
  }
  float fin = act ? score + end[j] : NEG;
  int idx = act ? j : 64;
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
  if (cnt >= 1) {  // history[t-1] belongs to step t; walk back over steps cnt-1 .. 1 (pytorch-crf: history[:seq_end])
    int cur = __builtin_amdgcn_readfirstlane(idx);
    path[cnt - 1] = cur;
    uint32_t word = bpw[((cnt - 1) >> 2) * 64 + j];
    for (int t = cnt - 1; t >= 1; --t) {
      if ((t & 3) == 3) word = bpw[(t >> 2) * 64 + j];
      cur = (lane_val((int)word, cur) >> (8 * (t & 3))) & 0xff;
      path[t - 1] = cur;
    }
  }
  __syncthreads();
  int32_t* out = tags_out + (long)b * S;
  for (int t = j; t < S; t += 64) out[t] = t < cnt ? path[t] : -1;
  if (j == 0) lens_out[b] = cnt;
}

}  // namespace crfw

static int crf_wide_ct(int C) { return C <= 32 ? 32 : (C <= 48 ? 48 : 64); }

size_t crf_wide_workspace_floats(int B, int S, int C) {
  const size_t CT = (size_t)crf_wide_ct(C), BS = (size_t)B * S;
  return 3 * BS * CT + BS + 2 * (size_t)B + (size_t)B * (2 * C + C * C);
}

CrfWideWs crf_wide_ws(void* ws, int B, int S, int C) {
  const size_t CT = (size_t)crf_wide_ct(C), BS = (size_t)B * S;
  CrfWideWs w;
  w.alpha = (float*)ws;
  w.sp = w.alpha + BS * CT;
  w.ui = w.sp + BS * CT;
  w.mx = w.ui + BS * CT;
  w.logz = w.mx + BS;
  w.llh = w.logz + B;
  w.partial = w.llh + B;
  return w;
}

#define CRFW_DISPATCH(C, LAUNCH) \
  switch (crf_wide_ct(C)) {      \
    case 32: LAUNCH(32); break;  \
    case 48: LAUNCH(48); break;  \
    default: LAUNCH(64); break;  \
  }

int crf_wide_fwd(const float* em, const int64_t* tags, const uint8_t* mask, const float* start, const float* end,
                 const float* trans, const CrfWideWs& w, int B, int S, int C, hipStream_t st) {
  const size_t lds = (size_t)S * (2 * sizeof(float) + sizeof(int) + 1);
#define L(CT) hipLaunchKernelGGL(HIP_KERNEL_NAME(crfw::crf_wide_fwd_kernel<CT, true>), dim3(B), dim3(64), lds, st, em, tags, \
                                 mask, start, end, trans, w.alpha, w.sp, w.mx, w.logz, w.llh, S, C)
  CRFW_DISPATCH(C, L)
#undef L
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

template <int GRAD>
static void crf_wide_bwd_launch(const float* gout, const float* em, const int64_t* tags, const uint8_t* mask,
                                const float* end, const float* trans, float* dem, const CrfWideWs& w, int B, int S, int C,
                                hipStream_t st) {
  const size_t lds = (size_t)S * (sizeof(float) + sizeof(int) + 1);
#define L(CT) hipLaunchKernelGGL(HIP_KERNEL_NAME(crfw::crf_wide_bwd_kernel<CT, GRAD>), dim3(B), dim3(64), lds, st, em, tags, \
                                 mask, end, trans, w.alpha, w.sp, w.mx, w.ui, gout, dem, w.partial, B, S, C)
  CRFW_DISPATCH(C, L)
#undef L
}

int crf_wide_bwd(int grad, const float* gout, const float* em, const int64_t* tags, const uint8_t* mask, const float* end,
                 const float* trans, float* dem, const CrfWideWs& w, int B, int S, int C, hipStream_t st) {
  if (grad == CRF_GRAD_SENTENCE) crf_wide_bwd_launch<CRF_GRAD_SENTENCE>(gout, em, tags, mask, end, trans, dem, w, B, S, C, st);
  else crf_wide_bwd_launch<CRF_GRAD_MEAN>(gout, em, tags, mask, end, trans, dem, w, B, S, C, st);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

int crf_wide_logz(const float* em, const uint8_t* mask, const float* start, const float* end, const float* trans,
                  const CrfWideWs& w, int B, int S, int C, hipStream_t st) {
  const size_t lds = (size_t)S * (2 * sizeof(float) + sizeof(int) + 1);
#define L(CT) hipLaunchKernelGGL(HIP_KERNEL_NAME(crfw::crf_wide_fwd_kernel<CT, false>), dim3(B), dim3(64), lds, st, em, \
                                 nullptr, mask, start, end, trans, w.alpha, w.sp, w.mx, w.logz, nullptr, S, C)
  CRFW_DISPATCH(C, L)
#undef L
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

int crf_wide_marginals(const float* em, const uint8_t* mask, const float* start, const float* end, const float* trans,
                       float* marg, const CrfWideWs& w, int B, int S, int C, hipStream_t st) {
  if (int rc = crf_wide_logz(em, mask, start, end, trans, w, B, S, C, st)) return rc;
  crf_wide_bwd_launch<CRF_MARGINALS>(nullptr, em, nullptr, mask, end, trans, marg, w, B, S, C, st);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

int crf_wide_viterbi(const float* em, const uint8_t* mask, const float* start, const float* end, const float* trans,
                     int32_t* tags_out, int32_t* lens_out, int B, int S, int C, hipStream_t st) {
  const size_t lds = (size_t)((S + 3) >> 2) * 64 * sizeof(uint32_t) + (size_t)S * (sizeof(int) + 1);
#define L(CT) hipLaunchKernelGGL(crfw::crf_wide_viterbi_kernel<CT>, dim3(B), dim3(64), lds, st, em, mask, start, end, \
                                 trans, tags_out, lens_out, S, C)
  CRFW_DISPATCH(C, L)
#undef L
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

#undef CRFW_DISPATCH

}  // namespace mtvaf
