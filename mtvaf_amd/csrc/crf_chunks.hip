// Tagger inference: the posterior of every CHUNK EVENT of a linear-chain CRF read through the tagging scheme, one launch.  Where
// crf_entities.hip reports log p(decoded segment | x) with the labels on either side marginalised, this reports, for every span
// of kept columns and every type, the probability that the chunker of entity.hip / crf_entities.hip (the reference's host chunker,
// modules/eval_metrics.py::get_chunks, on the tags of its decode, models/bert_model.py:511) would emit exactly that chunk:
//   post(b, w, T) = p( start at b,  no start at a kept column in (b, e],  end at e,  type_of[l_e] = T  |  x, y in A ),
// b = k_i, e = k_{i+w} the kept columns, under the chain over columns 0 .. L-1 restricted to the per-column tag sets A_t of
// crf_lattice.hip (0 = the full set), start and end included.  An end strictly inside the span does not exclude the event: the
// chunker emits both chunks then.
//
// A non-kept column strictly between two kept columns must carry a singleton set (the X of a sub-word piece); the kernel takes the
// lowest tag of A_t there, for every quantity it computes.  The weight G from one kept column to the next then factorises into a
// term of the source label, a scalar and a term of the destination label, and the state of the event recursion stays a vector over
// the last kept label:
//   open    g0_i(l')  = sum_l [start_tab[l][l']] alpha_{k_{i-1}}(l) G(l, l') em(l')      (i = 0: [start_tab[C][l']] alpha_{k_0}(l'))
//   extend  g^w(l')   = sum_l g^{w-1}(l) [not start_tab[l][l']] G(l, l') em(l')
//   close   post      = sum_{l: type_of[l] = T} g^w(l) eta_{i+w}(l) / Z_A
//   eta_j(l)          = sum_l'' [end_tab[l][l'']] G(l, l'') em(l'') beta_{k_{j+1}}(l'')    (j = n-1: [end_tab[l][C]] beta_{k_{n-1}}(l))
//
// One block of four wave64 per sentence, lane = tag, plain log domain (max-subtracted logsumexp), rows read across lanes with
// v_readlane, trans in the LDS with a row stride of 65 floats.  The two boolean tables are 64-bit masks in registers: lane l' holds
// column l' of start_tab (bit l = start_tab[l][l']), lane l row l of end_tab, lane T the labels of type T, so a masked term costs a
// shift and a select.  Wave 0 runs the backward sweep (beta over all columns; eta of every kept column and the three numbers of
// every gap) and the forward sweep (alpha; g0 of every kept column; logZ_A); g0 and eta go to a caller-provided global workspace,
// [B][S][64] floats each.  Then the four waves share the start columns: the running g row stays in one register per lane.  No
// atomics, no host read-back, every output element written.
#include "crf_chain.h"
#include "entity_bits.h"

namespace mtvaf {
namespace chk {

constexpr int MAX_S = CRF_CHAIN_SMAX;
constexpr int MAX_C = CRF_CHAIN_CMAX;
constexpr int MAX_W = 16;
constexpr int WORDS = MAX_S / 64;
constexpr int WAVES = 4;
constexpr int LD = CRF_CHAIN_LD;  // row stride of trans in the LDS: rows and columns both spread over the banks
constexpr int WS_LD = 64;         // floats per column in the workspace
constexpr int ADJ = 255;          // gap record of a kept column that follows the previous one directly

// log sum over i < C with bit i of m set of exp(x_i + row[i * stride]), x_i = lane i of x; -inf without a finite term
__device__ __forceinline__ float masked_lse(float x, const float* row, int stride, uint64_t m, int C) {
  const float NINF = -__builtin_inff();
  float mx = NINF;
  for (int i = 0; i < C; ++i) mx = fmaxf(mx, (m >> i) & 1 ? lane_val(x, i) + row[i * stride] : NINF);
  const float sh = mx == NINF ? 0.f : mx;
  float s = 0.f;
  for (int i = 0; i < C; ++i) s += (m >> i) & 1 ? __expf(lane_val(x, i) + row[i * stride] - sh) : 0.f;
  return mx == NINF ? NINF : sh + __logf(s);
}
// the same over x alone
__device__ __forceinline__ float masked_lse(float x, uint64_t m, int C) {
  const float NINF = -__builtin_inff();
  float mx = NINF;
  for (int i = 0; i < C; ++i) mx = fmaxf(mx, (m >> i) & 1 ? lane_val(x, i) : NINF);
  const float sh = mx == NINF ? 0.f : mx;
  float s = 0.f;
  for (int i = 0; i < C; ++i) s += (m >> i) & 1 ? __expf(lane_val(x, i) - sh) : 0.f;
  return mx == NINF ? NINF : sh + __logf(s);
}

__global__ __launch_bounds__(64 * WAVES) void crf_chunk_kernel(
    const float* __restrict__ em, const int64_t* __restrict__ allowed, const uint8_t* __restrict__ mask,
    const uint8_t* __restrict__ keep, const float* __restrict__ start, const float* __restrict__ end,
    const float* __restrict__ trans, const uint8_t* __restrict__ start_tab, const uint8_t* __restrict__ end_tab,
    const int* __restrict__ type_of, int n_types, int W, float* __restrict__ log_post, float* __restrict__ logz_a,
    float* __restrict__ ws_g0, float* __restrict__ ws_eta, int S, int C) {
  __shared__ float s_trans[MAX_C * LD];
  __shared__ uint64_t s_aw[MAX_S];      // the effective tag set of every column
  __shared__ uint64_t s_keep[WORDS];
  __shared__ float s_gs[MAX_S];         // by destination kept column: the scalar of the gap in front of it,
  __shared__ uint8_t s_gx1[MAX_S];      // the tag of the gap's first column (ADJ: no gap)
  __shared__ uint8_t s_gxg[MAX_S];      // and of its last
  __shared__ float s_logz;

  const float NINF = -__builtin_inff();
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, row = blockIdx.x;
  const int C1 = C + 1, nW = (S + 63) >> 6;
  stage_trans(s_trans, trans, C, tid, 64 * WAVES);
  const bool tag_lane = lane < C;
  const int jj = tag_lane ? lane : C - 1;  // lanes >= C compute on a valid address and are set to -inf afterwards
  const float start_l = start[jj], end_l = end[jj];
  uint64_t scol = 0, erow = 0, tmask = 0;
  for (int i = 0; i < C; ++i) {
    scol |= (uint64_t)(start_tab[i * C1 + jj] != 0) << i;
    erow |= (uint64_t)(end_tab[jj * C1 + i] != 0) << i;
    tmask |= (uint64_t)(min(max(type_of[i], 0), n_types - 1) == lane) << i;
  }
  const bool sb = start_tab[C * C1 + jj] != 0;  // a start behind the sentence boundary
  const bool eb = end_tab[jj * C1 + C] != 0;    // an end in front of it

  int L = S;  // leading ones of the mask
  for (int w = 0; w < nW; ++w) {
    const int c = lane + 64 * w;
    const uint64_t z = __ballot(c < S && mask[(long)row * S + c] == 0);
    if (z && L == S) L = 64 * w + __ffsll((long long)z) - 1;
  }
  if (wave == 0) {
    for (int w = 0; w < nW; ++w) {
      const int c = lane + 64 * w;
      const bool kp = c < L && (keep ? keep[(long)row * S + c] != 0 : c >= 1);
      const uint64_t kb = __ballot(kp);
      if (lane == 0) s_keep[w] = kb;
    }
  }
  __syncthreads();
  int k_first = -1;
  for (int w = nW - 1; w >= 0; --w)
    if (s_keep[w]) k_first = 64 * w + __ffsll((long long)s_keep[w]) - 1;
  const int k_last = ent_prev(s_keep, S - 1, true);
  const uint64_t full = C >= 64 ? ~0ull : (1ull << C) - 1ull;
  for (int t = tid; t < L; t += 64 * WAVES) {
    uint64_t a = allowed ? (uint64_t)allowed[(long)row * S + t] & full : full;
    if (!a) a = full;
    if (t > k_first && t < k_last && !(s_keep[t >> 6] >> (t & 63) & 1)) a &= ~a + 1;  // inside a gap: the lowest tag
    s_aw[t] = a;
  }
  __syncthreads();

  const float* emr = em + (long)row * S * C + jj;
  float* g0_w = ws_g0 + (long)row * S * WS_LD + lane;
  float* eta_w = ws_eta + (long)row * S * WS_LD + lane;

  if (wave == 0) {
    // backward sweep: on entry to column t, x = em_t+1(lane) + beta_t+1(lane) on A_t+1 and -inf outside
    float x = NINF, xk = NINF;  // xk: x of the next kept column nk
    int nk = -1, gx1 = -1, gxg = -1;
    float gs = 0.f;
    float en = L > 0 ? emr[(long)(L - 1) * C] : 0.f;
    for (int t = L - 1; t >= 0; --t) {
      const float et = en;
      if (t > 0) en = emr[(long)(t - 1) * C];
      const uint64_t A = s_aw[t];
      const bool ok = tag_lane && (A >> lane & 1);
      const bool kept = s_keep[t >> 6] >> (t & 63) & 1;
      const float b = t == L - 1 ? end_l : masked_lse(x, s_trans + jj * LD, 1, ~0ull, C);
      if (kept) {
        float eta;
        if (nk < 0)
          eta = eb ? b : NINF;
        else if (gx1 < 0)
          eta = masked_lse(xk, s_trans + jj * LD, 1, erow, C);
        else
          eta = masked_lse(xk, s_trans + gxg * LD, 1, erow, C) + (s_trans[jj * LD + gx1] + gs);
        eta_w[(long)t * WS_LD] = tag_lane ? eta : NINF;
        if (nk >= 0 && lane == 0) {
          s_gs[nk] = gs;
          s_gx1[nk] = (uint8_t)(gx1 < 0 ? ADJ : gx1);
          s_gxg[nk] = (uint8_t)(gxg < 0 ? ADJ : gxg);
        }
        nk = t;
        gx1 = gxg = -1;
        gs = 0.f;
      }
      x = ok ? b + et : NINF;
      if (kept) {
        xk = x;
      } else if (nk >= 0 && t > k_first) {  // a column of the gap in front of nk: its only tag
        const int xt = __ffsll((long long)A) - 1;
        gs += lane_val(et, xt);
        if (gxg < 0)
          gxg = xt;
        else
          gs += s_trans[xt * LD + gx1];  // gx1 is still the tag of column t + 1
        gx1 = xt;
      }
    }
  }
  __syncthreads();  // the gap records are in the LDS

  if (wave == 0) {
    // forward sweep: a = alpha_t(lane), aprev = alpha of the previous kept column
    float a = NINF, aprev = NINF;
    int pk = -1;
    float en = L > 0 ? emr[0] : 0.f;
    for (int t = 0; t < L; ++t) {
      const float et = en;
      if (t + 1 < L) en = emr[(long)(t + 1) * C];
      const uint64_t A = s_aw[t];
      const bool ok = tag_lane && (A >> lane & 1);
      const float v = (t == 0 ? start_l : masked_lse(a, s_trans + jj, LD, ~0ull, C)) + et;
      a = ok ? v : NINF;
      if (s_keep[t >> 6] >> (t & 63) & 1) {
        float g;
        if (pk < 0) {
          g = sb ? a : NINF;
        } else {
          const int gx1 = s_gx1[t];
          if (gx1 == ADJ)
            g = masked_lse(aprev, s_trans + jj, LD, scol, C) + et;
          else
            g = masked_lse(aprev, s_trans + gx1, LD, scol, C) + (s_gs[t] + s_trans[s_gxg[t] * LD + jj]) + et;
          g = ok ? g : NINF;
        }
        g0_w[(long)t * WS_LD] = g;
        aprev = a;
        pk = t;
      }
    }
    float logz = 0.f;
    if (L > 0) {
      const float xx = a + end_l;  // -inf outside the last set and on lanes >= C; the maximum is finite
      const float m = wave_max(xx);
      logz = m + __logf(wave_sum(__expf(xx - m)));
    }
    if (lane == 0) {
      s_logz = logz;
      logz_a[row] = logz;
    }
  }
  __syncthreads();  // g0 and eta are in the workspace (written and read inside this block), logZ_A in the LDS

  // the events: the waves share the start columns
  const double logz = (double)s_logz;
  float* out = log_post + (long)row * S * W * n_types;
  for (int b = wave; b < S; b += WAVES) {
    float* ob = out + (long)b * W * n_types;
    if (!(b < L && (s_keep[b >> 6] >> (b & 63) & 1))) {
      for (int i = lane; i < W * n_types; i += 64) ob[i] = NINF;
      continue;
    }
    float g = g0_w[(long)b * WS_LD];
    int col = b;
    for (int w = 0; w < W; ++w) {
      if (col < 0 || !__ballot(g > NINF)) {  // past the last kept column, or no path opens a chunk here and gets this far
        if (lane < n_types) ob[w * n_types + lane] = NINF;
        continue;
      }
      const float eta = eta_w[(long)col * WS_LD];
      // the two large terms cancel against logZ_A: taken in double, the difference adds no rounding of its own
      const float y = tag_lane ? (float)(((double)g + (double)eta) - logz) : NINF;
      const float p = masked_lse(y, tmask, C);
      if (lane < n_types) ob[w * n_types + lane] = p;
      if (w + 1 < W) {
        const int nc = ent_next(s_keep, col, nW);
        if (nc >= 0) {
          const bool ok = tag_lane && (s_aw[nc] >> lane & 1);
          const float e = emr[(long)nc * C];
          const int gx1 = s_gx1[nc];
          const float v = gx1 == ADJ ? masked_lse(g, s_trans + jj, LD, ~scol, C)
                                     : masked_lse(g, s_trans + gx1, LD, ~scol, C) + (s_gs[nc] + s_trans[s_gxg[nc] * LD + jj]);
          g = ok ? v + e : NINF;
        }
        col = nc;
      }
    }
  }
}

}  // namespace chk
}  // namespace mtvaf

using namespace mtvaf;

extern "C" {

size_t mtvaf_crf_chunk_posteriors_workspace_bytes(int B, int S, int C) {
  return bad_shape(B, S, C) ? 0 : (size_t)2 * B * S * chk::WS_LD * sizeof(float);
}

int mtvaf_crf_chunk_posteriors(const float* emissions, const int64_t* allowed, const uint8_t* mask, const uint8_t* keep,
                               const float* start, const float* end, const float* trans, const uint8_t* start_tab,
                               const uint8_t* end_tab, const int* type_of, int n_types, int max_width, float* log_post,
                               float* logz_a, int B, int S, int C, void* workspace, size_t workspace_bytes, hipStream_t st) {
  if (bad_shape(B, S, C)) return MTVAF_ERR_SHAPE;
  if (n_types < 1 || n_types > 64 || max_width < 1 || max_width > chk::MAX_W) return MTVAF_ERR_ARG;
  if (!workspace || workspace_bytes < mtvaf_crf_chunk_posteriors_workspace_bytes(B, S, C)) return MTVAF_ERR_WORKSPACE;
  float* g0 = (float*)workspace;
  float* eta = g0 + (size_t)B * S * chk::WS_LD;
  hipLaunchKernelGGL(chk::crf_chunk_kernel, dim3(B), dim3(64 * chk::WAVES), 0, st, emissions, allowed, mask, keep, start, end,
                     trans, start_tab, end_tab, type_of, n_types, max_width, log_post, logz_a, g0, eta, S, C);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

}  // extern "C"
