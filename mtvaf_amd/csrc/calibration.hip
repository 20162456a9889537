// Calibration of entity posteriors on the device: how often a chunk event (mtvaf_crf_chunk_posteriors' log_post) or a listed
// entity (mtvaf_crf_entities' ents / log_conf and the lists of the same format) of a given log-probability is a gold chunk.  One
// call ADDS, per entity type and log-probability bin, the scored items, the hits, sum p and sum (p - y)^2 of a batch -- and the
// gold chunks per type -- into a device counter block; precision / recall curves, the reliability table, ECE and the Brier
// score are a few host divisions on that block (mtvaf_amd/metrics.py: CalibrationScorer).
//
// Gold chunks: mtvaf_crf_entities' chunker on the gold labels (crf_entities.hip: kept columns keep, or 1 .. L-1 without one;
// a start at j iff start_tab[l_j-1][l_j], an end at j iff end_tab[l_j][l_j+1]; every end with a start b <= j closes
// (type_of[l_j], b, j), b the greatest such start; an end without a start is dropped), through the bit-set searches of
// entity_bits.h.  Every column ends at most one chunk, so the sentence's gold chunks are one LDS entry per END column (the start
// column, or -1); with the column of every kept ordinal beside it, "is (b, w, T) / (b, e, T) a gold chunk" is two LDS reads.
//
// Bins: the bin of lp is the number of k in 1 .. NB-1 with lp >= edges[k], on the fp32 values as stored: no exponential decides
// a bin, so a host that compares the same fp32 array agrees exactly.  p = exp((double)lp) enters only the two sums.
//
// One block (four wave64) per sentence.  Wave 0 chunks the gold labels: lane = column mod 64, flags are wave ballots parked in
// the LDS.  Then all four waves stride over the items (the S * W * T events, or the E slots).  Lanes of a wave that fall into the
// same (type, bin) cell are found by ballot, their p and (p - y)^2 summed in ascending lane order, and lane (cell mod 64) adds the
// result to the wave's own LDS cell -- always the same lane, in program order.  The cells of a pass (CAL_TILE of them: whole
// types, all bins) are summed over the four waves in wave order and STORED to the sentence's row of the workspace; a one-block
// pass then sums the rows in sentence order into the counter block.  No atomics on global memory, no floating-point atomics
// anywhere, integer LDS atomics for the gold counts only: the same inputs give the same bits.
#include "common.h"
#include "entity_bits.h"

namespace mtvaf {

constexpr int CAL_MAX_S = 512;
constexpr int CAL_MAX_C = 64;
constexpr int CAL_MAX_T = 64;
constexpr int CAL_MAX_W = 16;
constexpr int CAL_MAX_E = 64;
constexpr int CAL_MAX_NB = 64;
constexpr int CAL_WORDS = CAL_MAX_S / 64;
constexpr int CAL_WAVES = 4;
constexpr int CAL_THREADS = 64 * CAL_WAVES;
constexpr int CAL_TILE = 256;  // cells per pass: CAL_TILE / NB >= 4 whole types
enum { CAL_KEEP = 0, CAL_START = 1, CAL_SETS = 2 };

// 8-byte words of one sentence's workspace row = of the counter block without its last word (sentences)
__host__ __device__ inline long cal_row_words(int T, int NB) { return 4L * T * NB + 2L * T; }

// lane i's value of a double, i wave-uniform: two v_readlane
__device__ __forceinline__ double lane_f64(double x, int i) {
  const long long b = __double_as_longlong(x);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)b, i), hi = (unsigned)__builtin_amdgcn_readlane((int)(b >> 32), i);
  return __longlong_as_double((long long)((unsigned long long)hi << 32 | lo));
}

// One item per lane (valid: the lane has one): adds the wave's items cell by cell into the wave's LDS cells.  The lanes of a cell
// are summed in ascending lane order (a scalar loop over the ballot: every lane computes the same sum).
__device__ __forceinline__ void cal_accumulate(bool valid, int cell, double p, bool hit, int lane, unsigned* __restrict__ n,
                                               unsigned* __restrict__ h, double* __restrict__ sp, double* __restrict__ sq) {
  const double y = hit ? 1.0 : 0.0;
  const double d2 = (p - y) * (p - y);
  uint64_t todo = __ballot(valid);
  while (todo) {  // wave-uniform
    const int c = __builtin_amdgcn_readlane(cell, __ffsll((long long)todo) - 1);
    const bool mine = valid && cell == c;
    const uint64_t m = __ballot(mine);
    const unsigned nh = __popcll(__ballot(mine && hit));
    double a = 0.0, b = 0.0;
    for (uint64_t r = m; r; r &= r - 1) {
      const int l = __ffsll((long long)r) - 1;
      a += lane_f64(p, l);
      b += lane_f64(d2, l);
    }
    if (lane == (c & 63)) {
      n[c] += __popcll(m);
      h[c] += nh;
      sp[c] += a;
      sq[c] += b;
    }
    todo &= ~m;
  }
}

// DENSE: items are the elements of log_post [B,S,MW,T]; else the slots of ents [B,E,3] / log_conf [B,E].
template <bool DENSE>
__global__ __launch_bounds__(CAL_THREADS) void calibration_kernel(
    const float* __restrict__ log_post, const int* __restrict__ ents, const float* __restrict__ log_conf,
    const int64_t* __restrict__ gold, const uint8_t* __restrict__ mask, const uint8_t* __restrict__ keep,
    const uint8_t* __restrict__ start_tab, const uint8_t* __restrict__ end_tab, const int* __restrict__ type_of,
    const float* __restrict__ edges, int S, int C, int T, int MW, int E, int NB, unsigned long long* __restrict__ ws) {
  __shared__ uint8_t s_start[(CAL_MAX_C + 1) * (CAL_MAX_C + 1)], s_end[(CAL_MAX_C + 1) * (CAL_MAX_C + 1)];
  __shared__ int s_type[CAL_MAX_C + 1];
  __shared__ float s_edges[CAL_MAX_NB + 1];
  __shared__ uint8_t s_lab[CAL_MAX_S];               // sanitised gold labels
  __shared__ uint64_t s_bits[CAL_SETS][CAL_WORDS];
  __shared__ int s_kbase[CAL_WORDS];                 // kept columns before word w
  __shared__ short s_kcol[CAL_MAX_S];                // column of the kept ordinal o
  __shared__ short s_gstart[CAL_MAX_S];              // per END column: the start column of the gold chunk, or -1
  __shared__ unsigned s_gold[CAL_MAX_T], s_reach[CAL_MAX_T];
  __shared__ int s_nkept;
  __shared__ unsigned s_n[CAL_WAVES][CAL_TILE], s_h[CAL_WAVES][CAL_TILE];
  __shared__ double s_sp[CAL_WAVES][CAL_TILE], s_sq[CAL_WAVES][CAL_TILE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long row = blockIdx.x;
  const int C1 = C + 1, NW = (S + 63) >> 6;
  for (int i = tid; i < C1 * C1; i += CAL_THREADS) {
    s_start[i] = start_tab[i];
    s_end[i] = end_tab[i];
  }
  for (int i = tid; i < C1; i += CAL_THREADS) s_type[i] = min(max(type_of[i], 0), T - 1);
  for (int i = tid; i <= NB; i += CAL_THREADS) s_edges[i] = edges[i];
  for (int i = tid; i < T; i += CAL_THREADS) s_gold[i] = s_reach[i] = 0;

  // ---- wave 0: the gold chunks of the sentence (the barriers are block-wide, so the other waves walk along) ----
  if (wave == 0) {
    int L = S;  // leading ones of the mask
    for (int w = 0; w < NW; ++w) {
      const int c = lane + 64 * w;
      const uint64_t z = __ballot(c < S && mask[row * S + c] == 0);
      if (z && L == S) L = 64 * w + __ffsll((long long)z) - 1;
    }
    int nk = 0;  // kept columns so far (wave-uniform)
    for (int w = 0; w < NW; ++w) {
      const int c = lane + 64 * w;
      bool kp = false;
      int l = 0;
      if (c < L) {
        const int64_t g = gold[row * S + c];
        l = g >= 0 && g < C ? (int)g : 0;
        kp = keep ? keep[row * S + c] != 0 : c >= 1;
      }
      s_lab[c] = (uint8_t)l;  // c < 64 NW <= CAL_MAX_S
      s_gstart[c] = -1;
      const uint64_t kb = __ballot(kp);
      if (kp) s_kcol[nk + __popcll(kb & ((1ull << lane) - 1))] = (short)c;
      if (lane == 0) {
        s_bits[CAL_KEEP][w] = kb;
        s_kbase[w] = nk;
      }
      nk += __popcll(kb);
    }
    if (lane == 0) s_nkept = nk;
  }
  __syncthreads();  // tables, labels and the keep words are in the LDS

  unsigned ends = 0;  // wave 0, bit w: this lane's column lane + 64 w ends a chunk
  if (wave == 0) {
    for (int w = 0; w < NW; ++w) {
      const int c = lane + 64 * w;
      bool st = false, en = false;
      if (s_bits[CAL_KEEP][w] >> lane & 1) {
        const int pc = ent_prev(s_bits[CAL_KEEP], c, false), nc = ent_next(s_bits[CAL_KEEP], c, NW);
        const int l = s_lab[c], lprev = pc >= 0 ? s_lab[pc] : C, lnext = nc >= 0 ? s_lab[nc] : C;
        st = s_start[lprev * C1 + l] != 0;
        en = s_end[l * C1 + lnext] != 0;
      }
      const uint64_t sb = __ballot(st);
      if (lane == 0) s_bits[CAL_START][w] = sb;
      ends |= (unsigned)en << w;
    }
  }
  __syncthreads();  // the start words are in the LDS

  if (wave == 0) {
    for (int w = 0; w < NW; ++w) {
      if (!(ends >> w & 1)) continue;
      const int c = lane + 64 * w;
      const int b = ent_prev(s_bits[CAL_START], c, true);
      if (b < 0) continue;  // an end without a start is dropped
      s_gstart[c] = (short)b;
      const int t = s_type[s_lab[c]];
      atomicAdd(&s_gold[t], 1u);
      // width in kept columns: ordinal of c minus ordinal of b, plus one (both are kept columns)
      const int oc = s_kbase[w] + __popcll(s_bits[CAL_KEEP][w] & ((1ull << lane) - 1));
      const int ob = s_kbase[b >> 6] + __popcll(s_bits[CAL_KEEP][b >> 6] & ((1ull << (b & 63)) - 1));
      if (!DENSE || oc - ob < MW) atomicAdd(&s_reach[t], 1u);
    }
  }
  __syncthreads();  // the gold chunks are in the LDS

  // ---- all waves: the items, CAL_TILE cells (whole types) per pass ----
  unsigned long long* out = ws + row * cal_row_words(T, NB);
  const int cells = T * NB, TT = CAL_TILE / NB;  // NB <= 64: TT >= 4
  const int nkept = s_nkept;
  for (int t0 = 0; t0 < T; t0 += TT) {
    const int nt = min(TT, T - t0), ncell = nt * NB;
    for (int c = lane; c < ncell; c += 64) {  // the lane that owns the cell
      s_n[wave][c] = s_h[wave][c] = 0;
      s_sp[wave][c] = s_sq[wave][c] = 0.0;
    }
    const int n_items = DENSE ? S * MW * nt : E;
    for (int base = wave * 64; base < n_items; base += CAL_THREADS) {  // wave-uniform
      const int j = base + lane;
      bool valid = false, hit = false;
      int cell = 0;
      double p = 0.0;
      if (j < n_items) {
        float lp = 0.f;
        int b = 0, e = -1, t = 0;
        bool dead = false;  // a listed slot without a usable confidence: bin 0, p = 0
        if (DENSE) {
          const int pos = j / nt, w = pos % MW;  // pos = b * MW + w
          b = pos / MW;
          t = t0 + (j - pos * nt);
          lp = log_post[(row * S * MW + pos) * T + t];
          valid = lp > -INFINITY;  // false for NaN
          if (valid && (s_bits[CAL_KEEP][b >> 6] >> (b & 63) & 1)) {
            const int o = s_kbase[b >> 6] + __popcll(s_bits[CAL_KEEP][b >> 6] & ((1ull << (b & 63)) - 1)) + w;
            if (o < nkept) e = s_kcol[o];
          }
        } else {
          const int* en = ents + (row * E + j) * 3;
          b = en[0];
          e = en[1];
          t = en[2];
          valid = b >= 0 && b < S && e >= 0 && e < S && t >= t0 && t < t0 + nt;  // t0 + nt <= T
          lp = log_conf[row * E + j];
          dead = !(lp > -INFINITY);
          if (!valid) e = -1;
        }
        if (valid) {
          hit = e >= 0 && s_gstart[e] == b && s_type[s_lab[e]] == t;
          int bin = 0;
          if (!dead) {
            for (int k = 1; k < NB; ++k) bin += lp >= s_edges[k];
            p = exp((double)lp);
          }
          cell = (t - t0) * NB + bin;
        }
      }
      cal_accumulate(valid, cell, p, hit, lane, s_n[wave], s_h[wave], s_sp[wave], s_sq[wave]);
    }
    __syncthreads();  // the four waves' cells of this pass are complete
    for (int c = tid; c < ncell; c += CAL_THREADS) {
      unsigned long long n = 0, h = 0;
      double a = 0.0, q = 0.0;
#pragma unroll
      for (int v = 0; v < CAL_WAVES; ++v) {
        n += s_n[v][c];
        h += s_h[v][c];
        a += s_sp[v][c];
        q += s_sq[v][c];
      }
      const int g = t0 * NB + c;
      out[g] = n;
      out[cells + g] = h;
      out[2 * cells + 2 * T + g] = (unsigned long long)__double_as_longlong(a);
      out[3 * cells + 2 * T + g] = (unsigned long long)__double_as_longlong(q);
    }
    __syncthreads();  // the next pass clears the cells
  }
  for (int t = tid; t < T; t += CAL_THREADS) {
    out[2 * cells + t] = s_gold[t];
    out[2 * cells + T + t] = s_reach[t];
  }
}

// One block: counter[i] += sum over the sentences, in sentence order, of workspace row b's word i; sentences += B.
__global__ __launch_bounds__(CAL_THREADS) void calibration_reduce_kernel(const unsigned long long* __restrict__ ws, int B, int T,
                                                                         int NB, unsigned long long* __restrict__ counter) {
  const long words = cal_row_words(T, NB), f64_from = 2L * T * NB + 2L * T;  // the two double tables are the row's tail
  for (long i = threadIdx.x; i < words; i += CAL_THREADS) {
    if (i >= f64_from) {
      double s = 0.0;
      for (int b = 0; b < B; ++b) s += __longlong_as_double((long long)ws[b * words + i]);
      counter[i] = (unsigned long long)__double_as_longlong(__longlong_as_double((long long)counter[i]) + s);
    } else {
      unsigned long long s = 0;
      for (int b = 0; b < B; ++b) s += ws[b * words + i];
      counter[i] += s;
    }
  }
  if (threadIdx.x == 0) counter[words] += (unsigned long long)B;
}

static int cal_check(int B, int S, int C, int T, int MW, int E, int NB, const void* workspace, size_t workspace_bytes) {
  if (B <= 0 || S < 1 || S > CAL_MAX_S || C < 1 || C > CAL_MAX_C) return MTVAF_ERR_SHAPE;
  if (T < 1 || T > CAL_MAX_T || MW < 1 || MW > CAL_MAX_W || E < 1 || E > CAL_MAX_E || NB < 1 || NB > CAL_MAX_NB)
    return MTVAF_ERR_ARG;
  if (!workspace || workspace_bytes < mtvaf_calibration_workspace_bytes(B, T, NB)) return MTVAF_ERR_WORKSPACE;
  return MTVAF_OK;
}

}  // namespace mtvaf

using namespace mtvaf;

extern "C" {

size_t mtvaf_calibration_workspace_bytes(int B, int n_types, int n_bins) {
  if (B <= 0 || n_types < 1 || n_types > CAL_MAX_T || n_bins < 1 || n_bins > CAL_MAX_NB) return 0;
  return (size_t)B * (size_t)cal_row_words(n_types, n_bins) * 8;
}

int mtvaf_chunk_calibration(const float* log_post, const int64_t* gold, const uint8_t* mask, const uint8_t* keep,
                            const uint8_t* start_tab, const uint8_t* end_tab, const int* type_of, const float* edges, int B,
                            int S, int C, int n_types, int max_width, int n_bins, void* counter, void* workspace,
                            size_t workspace_bytes, hipStream_t st) {
  const int rc = cal_check(B, S, C, n_types, max_width, 1, n_bins, workspace, workspace_bytes);
  if (rc != MTVAF_OK) return rc;
  hipLaunchKernelGGL(calibration_kernel<true>, dim3(B), dim3(CAL_THREADS), 0, st, log_post, nullptr, nullptr, gold, mask, keep,
                     start_tab, end_tab, type_of, edges, S, C, n_types, max_width, 0, n_bins, (unsigned long long*)workspace);
  MTVAF_LAUNCH_CHECK();
  hipLaunchKernelGGL(calibration_reduce_kernel, dim3(1), dim3(CAL_THREADS), 0, st, (const unsigned long long*)workspace, B,
                     n_types, n_bins, (unsigned long long*)counter);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

int mtvaf_entity_calibration(const int32_t* ents, const float* log_conf, const int64_t* gold, const uint8_t* mask,
                             const uint8_t* keep, const uint8_t* start_tab, const uint8_t* end_tab, const int* type_of,
                             const float* edges, int B, int S, int C, int n_types, int max_entities, int n_bins, void* counter,
                             void* workspace, size_t workspace_bytes, hipStream_t st) {
  const int rc = cal_check(B, S, C, n_types, 1, max_entities, n_bins, workspace, workspace_bytes);
  if (rc != MTVAF_OK) return rc;
  hipLaunchKernelGGL(calibration_kernel<false>, dim3(B), dim3(CAL_THREADS), 0, st, nullptr, ents, log_conf, gold, mask, keep,
                     start_tab, end_tab, type_of, edges, S, C, n_types, 1, max_entities, n_bins, (unsigned long long*)workspace);
  MTVAF_LAUNCH_CHECK();
  hipLaunchKernelGGL(calibration_reduce_kernel, dim3(1), dim3(CAL_THREADS), 0, st, (const unsigned long long*)workspace, B,
                     n_types, n_bins, (unsigned long long*)counter);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

}  // extern "C"
