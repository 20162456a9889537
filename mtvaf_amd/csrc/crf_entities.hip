// Tagger inference: the entities of decoded tag sequences with the CRF posterior of each decoded segment, one launch.  It
// complements the reference's decode (models/bert_model.py:511) and its host chunker (modules/eval_metrics.py::get_chunks): the
// chunks are emitted, not counted, and each carries
//   log_conf = alpha_b(t_b) + sum_{k=b+1..e} (trans[t_k-1][t_k] + em_k[t_k]) + beta_e(t_e) - logZ
// over ALL columns b..e of the chunk (kept or not), alpha / beta / logZ of the unconstrained chain over columns 0 .. L-1 of the
// sentence (start and end included): log p(y_b..y_e = decoded tags | x), the labels on either side marginalised.
//
// Chunk rule: one side of entity.hip's.  Over the kept columns (keep, or 1 .. L-1 without one) and their sanitised labels l_j, with
// the sentence boundary C on both sides: a start at j iff start_tab[l_j-1][l_j], an end at j iff end_tab[l_j][l_j+1]; every end
// with a start b <= j closes (type_of[l_j], b, j), b the greatest such start; an end without a start is dropped.
//
// One wave64 per sentence, four sentences per block.  Chunking: lane = column mod 64, flags are wave ballots (one 64-bit word per 64
// columns, in the LDS).  Recursions: lane = tag, plain log domain (max-subtracted logsumexp), a full alpha / beta row lives in one
// register per lane and is read across lanes with v_readlane; lanes >= C carry -inf and are never read.  The sweeps leave two numbers
// per column in the LDS, alpha_t(tag_t) and beta_t(tag_t); emissions pass through a 16-column LDS window filled by coalesced loads.
// No workspace, no atomics, every output element written: slot numbers are prefix counts of the end ballots.
#include "crf_chain.h"
#include "entity_bits.h"

namespace mtvaf {

constexpr int CE_MAX_S = CRF_CHAIN_SMAX;
constexpr int CE_MAX_C = CRF_CHAIN_CMAX;
constexpr int CE_MAX_E = 64;                  // slots per sentence: one per lane when the unused ones are filled
constexpr int CE_WORDS = CE_MAX_S / 64;
constexpr int CE_WAVES = 4;                   // sentences in flight per block
constexpr int CE_LD = CRF_CHAIN_LD;           // row stride of trans in the LDS: rows (backward) and columns (forward) both hit 32 banks
constexpr int CE_WIN = 16;                    // columns of emissions per LDS window
enum { CE_KEEP = 0, CE_START = 1, CE_SETS = 2 };

// log sum_i exp(x_i + row[i * stride]) over i < C, x_i = lane i of x; every term finite
__device__ __forceinline__ float ce_lse(float x, const float* row, int stride, int C) {
  float m = -INFINITY;
  for (int i = 0; i < C; ++i) m = fmaxf(m, lane_val(x, i) + row[i * stride]);
  float s = 0.f;
  for (int i = 0; i < C; ++i) s += __expf(lane_val(x, i) + row[i * stride] - m);
  return m + __logf(s);
}

__global__ __launch_bounds__(64 * CE_WAVES) void crf_entities_kernel(
    const float* __restrict__ em, const uint8_t* __restrict__ mask, const int* __restrict__ tags, int ldt,
    const uint8_t* __restrict__ keep, const float* __restrict__ start, const float* __restrict__ end,
    const float* __restrict__ trans, const uint8_t* __restrict__ start_tab, const uint8_t* __restrict__ end_tab,
    const int* __restrict__ type_of, int n_types, int* __restrict__ ents, float* __restrict__ log_conf,
    int* __restrict__ count, int B, int S, int C, int max_entities) {
  __shared__ float s_trans[CE_MAX_C * CE_LD];
  __shared__ uint8_t s_start[(CE_MAX_C + 1) * (CE_MAX_C + 1)], s_end[(CE_MAX_C + 1) * (CE_MAX_C + 1)];
  __shared__ int s_type[CE_MAX_C + 1];
  __shared__ float s_em[CE_WAVES][CE_WIN * CE_MAX_C];
  __shared__ float s_atag[CE_WAVES][CE_MAX_S], s_btag[CE_WAVES][CE_MAX_S];  // alpha_t(tag_t), beta_t(tag_t)
  __shared__ uint8_t s_lab[CE_WAVES][CE_MAX_S];                              // sanitised decoded tags
  __shared__ uint64_t s_bits[CE_WAVES][CE_SETS][CE_WORDS];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int C1 = C + 1, W = (S + 63) >> 6, n_win = (S + CE_WIN - 1) / CE_WIN;
  stage_trans(s_trans, trans, C, tid, 64 * CE_WAVES);
  for (int i = tid; i < C1 * C1; i += 64 * CE_WAVES) {
    s_start[i] = start_tab[i];
    s_end[i] = end_tab[i];
  }
  for (int i = tid; i < C1; i += 64 * CE_WAVES) s_type[i] = min(max(type_of[i], 0), n_types - 1);
  const bool tag_lane = lane < C;
  const int jj = tag_lane ? lane : C - 1;  // lanes >= C compute on a valid address and are set to -inf afterwards
  const float start_l = start[jj], end_l = end[jj];
  __syncthreads();

  uint8_t* lab = s_lab[wave];
  float* atag = s_atag[wave];
  float* btag = s_btag[wave];
  float* win = s_em[wave];
  uint64_t(*bits)[CE_WORDS] = s_bits[wave];

  // every wave of the block makes the same number of trips: the barriers below are block-wide
  for (int base = blockIdx.x * CE_WAVES; base < B; base += gridDim.x * CE_WAVES) {
    const int row = base + wave;
    const bool active = row < B;  // wave-uniform
    int L = 0;                    // leading ones of the mask
    if (active) {
      L = S;
      for (int w = 0; w < W; ++w) {
        const int c = lane + 64 * w;
        const uint64_t z = __ballot(c < S && mask[(long)row * S + c] == 0);
        if (z && L == S) L = 64 * w + __ffsll((long long)z) - 1;
      }
      for (int w = 0; w < W; ++w) {
        const int c = lane + 64 * w;
        bool kp = false;
        int l = 0;
        if (c < L) {
          const int t = tags[(long)row * ldt + c];
          l = t >= 0 && t < C ? t : 0;
          kp = keep ? keep[(long)row * S + c] != 0 : c >= 1;
        }
        lab[c] = (uint8_t)l;  // c < 64 W <= CE_MAX_S
        const uint64_t kb = __ballot(kp);
        if (lane == 0) bits[CE_KEEP][w] = kb;
      }
    }
    __syncthreads();  // labels and the keep words are in the LDS

    unsigned ends = 0;  // bit w: this lane's column lane + 64 w ends a chunk
    if (active) {
      for (int w = 0; w < W; ++w) {
        const int c = lane + 64 * w;
        bool st = false, en = false;
        if (bits[CE_KEEP][w] >> lane & 1) {
          const int pc = ent_prev(bits[CE_KEEP], c, false), nc = ent_next(bits[CE_KEEP], c, W);
          const int l = lab[c], lprev = pc >= 0 ? lab[pc] : C, lnext = nc >= 0 ? lab[nc] : C;
          st = s_start[lprev * C1 + l] != 0;
          en = s_end[l * C1 + lnext] != 0;
        }
        const uint64_t sb = __ballot(st);
        if (lane == 0) bits[CE_START][w] = sb;
        ends |= (unsigned)en << w;
      }
    }

    // forward sweep: a = alpha_t(lane); window k holds the emissions of columns 16 k .. 16 k + 15
    float a = -INFINITY, logz = 0.f;
    for (int k = 0; k < n_win; ++k) {
      const int t0 = k * CE_WIN, n = min(CE_WIN, L - t0);  // n <= 0: the sentence has ended (or the wave has none)
      const float* src = em + ((long)row * S + t0) * C;
      for (int i = lane; i < n * C; i += 64) win[i] = src[i];
      __syncthreads();
      for (int t = t0; t < t0 + n; ++t) {
        const float v = (t == 0 ? start_l : ce_lse(a, s_trans + jj, CE_LD, C)) + win[(t - t0) * C + jj];
        a = tag_lane ? v : -INFINITY;
        if (lane == lab[t]) atag[t] = a;
      }
      __syncthreads();  // the next window overwrites this one
    }
    if (L > 0) {
      const float x = a + end_l;  // -inf on lanes >= C: exp(-inf - m) = 0, and m is finite (C >= 1)
      const float m = wave_max(x);
      logz = m + __logf(wave_sum(__expf(x - m)));
    }

    // backward sweep: on entry to column t, x = em_t+1(lane) + beta_t+1(lane) (made while column t + 1 was in the window)
    float x = -INFINITY;
    for (int k = n_win - 1; k >= 0; --k) {
      const int t0 = k * CE_WIN, n = min(CE_WIN, L - t0);
      const float* src = em + ((long)row * S + t0) * C;
      for (int i = lane; i < n * C; i += 64) win[i] = src[i];
      __syncthreads();
      for (int t = t0 + n - 1; t >= t0; --t) {
        const float v = t == L - 1 ? end_l : ce_lse(x, s_trans + jj * CE_LD, 1, C);
        const float b = tag_lane ? v : -INFINITY;
        if (lane == lab[t]) btag[t] = b;
        x = b + win[(t - t0) * C + jj];
      }
      __syncthreads();  // also: the start words, atag and btag are in the LDS
    }

    if (active) {
      int total = 0;  // chunks found so far (wave-uniform)
      for (int w = 0; w < W; ++w) {
        const int c = lane + 64 * w;
        const int b = ends >> w & 1 ? ent_prev(bits[CE_START], c, true) : -1;
        const uint64_t vb = __ballot(b >= 0);
        const int slot = total + __popcll(vb & ((1ull << lane) - 1));
        total += __popcll(vb);
        if (b >= 0 && slot < max_entities) {
          float path = 0.f;
          int lp = lab[b];
          for (int k = b + 1; k <= c; ++k) {
            const int l = lab[k];
            path += s_trans[lp * CE_LD + l] + em[((long)row * S + k) * C + l];
            lp = l;
          }
          // the three large terms cancel to the size of the result: taken in double, they add no rounding of their own
          const double lc = ((double)atag[b] + (double)btag[c] - (double)logz) + (double)path;
          const long o = (long)row * max_entities + slot;
          ents[o * 3 + 0] = b;
          ents[o * 3 + 1] = c;
          ents[o * 3 + 2] = s_type[lab[c]];
          log_conf[o] = (float)lc;
        }
      }
      if (lane < max_entities && lane >= total) {  // max_entities <= 64: one unused slot per lane
        const long o = (long)row * max_entities + lane;
        ents[o * 3 + 0] = -1;
        ents[o * 3 + 1] = -1;
        ents[o * 3 + 2] = -1;
        log_conf[o] = 0.f;
      }
      if (lane == 0) count[row] = total;
    }
    __syncthreads();  // the next sentence overwrites labels, words and the per-column numbers
  }
}

}  // namespace mtvaf

using namespace mtvaf;

extern "C" {

int mtvaf_crf_entities(const float* emissions, const uint8_t* mask, const int32_t* tags, int ldt, const uint8_t* keep,
                       const float* start, const float* end, const float* trans, const uint8_t* start_tab,
                       const uint8_t* end_tab, const int* type_of, int n_types, int32_t* ents, float* log_conf,
                       int32_t* count, int B, int S, int C, int max_entities, hipStream_t st) {
  if (bad_shape(B, S, C) || ldt < S) return MTVAF_ERR_SHAPE;
  if (n_types < 1 || n_types > C + 1 || max_entities < 1 || max_entities > CE_MAX_E) return MTVAF_ERR_ARG;
  const int blocks = min((B + CE_WAVES - 1) / CE_WAVES, 1024);
  hipLaunchKernelGGL(crf_entities_kernel, dim3(blocks), dim3(64 * CE_WAVES), 0, st, emissions, mask, tags, ldt, keep, start, end,
                     trans, start_tab, end_tab, type_of, n_types, ents, log_conf, count, B, S, C, max_entities);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

}  // extern "C"
