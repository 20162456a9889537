// Entity-level scoring of decoded tag sequences on the device: the counting half of the reference trainer's score
// (modules/train.py:627-647, :714-731 build y_true / y_pred on the host; modules/eval_metrics.py::get_chunks / evaluate /
// evaluate_each_class and seqeval's classification_report chunk and count them).  One launch ADDS, per entity type, the
// predicted, gold and correct chunks of a batch -- and the equal / kept token counts -- into a 64-bit device counter.
//
// The rule is exact on integers and knows no tagging scheme: the scheme is the two tables.  Per sentence:
//   kept columns   1 .. S-1 while mask is 1 (the reference stops at the first 0), minus those whose gold label is skipped
//                  (gold_skip); both label sequences share this set.  A label id outside [0, C) reads as 0.
//   events         per side (gold / pred) over the kept labels l_j, with l_-1 = l_n = C (the sentence boundary):
//                  a start at j iff start_tab[l_j-1][l_j], an end at j iff end_tab[l_j][l_j+1].  Every end closes one chunk
//                  (type_of[l_j], b, j), b = the greatest start <= j of the sentence; without one the chunk is unopened: it is
//                  counted for its type and never correct.
//   correct        both sides end at j, both chunks are opened at the same b, both have the same type.
// Both sides share the kept set, so column coordinates stand in for positions in the compacted sequences: nothing is compacted.
//
// One wave64 per sentence, lane = column mod 64 (up to 8 columns per lane).  Keep / start / end flags are wave ballots, one 64-bit
// word per 64 columns, parked in the LDS next to the sanitised labels; "previous / next kept column" and "last start <= j" are
// highest / lowest-set-bit searches over those words.  Counts go through LDS integer atomics per block and leave as one 64-bit
// global atomic per block and non-zero counter: integer sums commute, so the counter is bit-reproducible.
//
// ROWS = true (mtvaf_entity_counts_rows) runs the same chunking per row and writes (predicted, gold, correct) of row r, summed
// over the types, to rows_out[r]: row r is scored against gold / mask row r / group, so K hypotheses of one sentence share its
// gold row.  No global counter, no token counts.
#include "common.h"
#include "entity_bits.h"

namespace mtvaf {

constexpr int ENT_MAX_S = 512;
constexpr int ENT_MAX_C = 64;
constexpr int ENT_WORDS = ENT_MAX_S / 64;
constexpr int ENT_WAVES = 4;                       // sentences in flight per block
constexpr int ENT_MAX_T = ENT_MAX_C + 1;           // type_of has C + 1 entries: no more types than that
constexpr int ENT_MAX_CNT = ENT_MAX_T * 3 + 2;
enum { ENT_KEEP = 0, ENT_START = 1, ENT_END = 3, ENT_SETS = 5 };  // bit sets of a sentence: keep, start[2], end[2]

template <bool ROWS>
__global__ __launch_bounds__(64 * ENT_WAVES) void entity_counts_kernel(
    const int* __restrict__ pred, int ldp, const int64_t* __restrict__ gold, const uint8_t* __restrict__ mask,
    const uint8_t* __restrict__ start_tab, const uint8_t* __restrict__ end_tab, const int* __restrict__ type_of,
    const uint8_t* __restrict__ gold_skip, int B, int S, int C, int n_types, unsigned long long* __restrict__ counts,
    int group, int32_t* __restrict__ rows_out) {
  __shared__ uint8_t s_start[(ENT_MAX_C + 1) * (ENT_MAX_C + 1)], s_end[(ENT_MAX_C + 1) * (ENT_MAX_C + 1)];
  __shared__ int s_type[ENT_MAX_C + 1];
  __shared__ uint8_t s_skip[ENT_MAX_C];
  __shared__ uint8_t s_lab[ENT_WAVES][2][ENT_MAX_S];       // sanitised labels of the wave's sentence: [0] gold, [1] pred
  __shared__ uint64_t s_bits[ENT_WAVES][ENT_SETS][ENT_WORDS];
  __shared__ unsigned s_cnt[ENT_MAX_CNT];
  __shared__ unsigned s_row[ENT_WAVES][3];                 // ROWS: predicted, gold, correct of the wave's row

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int C1 = C + 1, n_cnt = n_types * 3 + 2, W = (S + 63) >> 6;
  for (int i = tid; i < C1 * C1; i += 64 * ENT_WAVES) {
    s_start[i] = start_tab[i];
    s_end[i] = end_tab[i];
  }
  for (int i = tid; i < C1; i += 64 * ENT_WAVES) s_type[i] = min(max(type_of[i], 0), n_types - 1);
  for (int i = tid; i < C; i += 64 * ENT_WAVES) s_skip[i] = gold_skip[i];
  for (int i = tid; i < n_cnt; i += 64 * ENT_WAVES) s_cnt[i] = 0;
  __syncthreads();

  uint8_t* lab_g = s_lab[wave][0];
  uint8_t* lab_p = s_lab[wave][1];
  uint64_t(*bits)[ENT_WORDS] = s_bits[wave];

  // every wave of the block makes the same number of trips: the barriers below are block-wide
  for (int base = blockIdx.x * ENT_WAVES; base < B; base += gridDim.x * ENT_WAVES) {
    const int row = base + wave;
    const bool active = row < B;  // wave-uniform
    const long grow = ROWS ? row / group : row;  // the gold / mask row
    if (ROWS && lane < 3) s_row[wave][lane] = 0;
    if (active) {
      // the run of mask 1 from column 1: ends at the first 0
      int run_end = S;
      for (int w = 0; w < W; ++w) {
        const int c = lane + 64 * w;
        const bool zero = c >= 1 && c < S && mask[grow * S + c] == 0;
        const uint64_t z = __ballot(zero);
        if (z && run_end == S) run_end = 64 * w + __ffsll((long long)z) - 1;
      }
      unsigned n_kept = 0, n_equal = 0;
      for (int w = 0; w < W; ++w) {
        const int c = lane + 64 * w;
        bool keep = false;
        int lg = 0, lp = 0;
        if (c >= 1 && c < run_end) {
          const int64_t g = gold[grow * S + c];
          const int p = pred[(long)row * ldp + c];
          const bool g_in = g >= 0 && g < C;
          lg = g_in ? (int)g : 0;
          lp = p >= 0 && p < C ? p : 0;
          keep = !(g_in && s_skip[lg]);
        }
        lab_g[c] = (uint8_t)lg;  // c < 64 W <= ENT_MAX_S
        lab_p[c] = (uint8_t)lp;
        const uint64_t kb = __ballot(keep);
        const uint64_t eq = __ballot(keep && lg == lp);
        if (lane == 0) bits[ENT_KEEP][w] = kb;
        n_kept += __popcll(kb);
        n_equal += __popcll(eq);
      }
      if (!ROWS && lane == 0) {
        if (n_equal) atomicAdd(&s_cnt[n_types * 3], n_equal);
        if (n_kept) atomicAdd(&s_cnt[n_types * 3 + 1], n_kept);
      }
    }
    __syncthreads();  // labels and the keep words are in the LDS

    unsigned ends = 0;  // bit 2 w + side: this lane's column lane + 64 w closes a chunk on that side
    if (active) {
      for (int w = 0; w < W; ++w) {
        const int c = lane + 64 * w;
        const bool keep = bits[ENT_KEEP][w] >> lane & 1;
        bool st[2] = {false, false}, en[2] = {false, false};
        if (keep) {
          const int pc = ent_prev(bits[ENT_KEEP], c, false), nc = ent_next(bits[ENT_KEEP], c, W);
#pragma unroll
          for (int side = 0; side < 2; ++side) {
            const uint8_t* lab = side ? lab_p : lab_g;
            const int l = lab[c], lprev = pc >= 0 ? lab[pc] : C, lnext = nc >= 0 ? lab[nc] : C;
            st[side] = s_start[lprev * C1 + l] != 0;
            en[side] = s_end[l * C1 + lnext] != 0;
          }
        }
#pragma unroll
        for (int side = 0; side < 2; ++side) {
          const uint64_t sb = __ballot(st[side]);
          if (lane == 0) bits[ENT_START + side][w] = sb;
          ends |= (unsigned)en[side] << (2 * w + side);
        }
      }
    }
    __syncthreads();  // the start words are in the LDS

    if (active) {
      for (int w = 0; w < W; ++w) {
        const unsigned e = ends >> (2 * w) & 3;
        if (!e) continue;
        const int c = lane + 64 * w;
        const int tg = s_type[lab_g[c]], tp = s_type[lab_p[c]];
        if (e & 1) atomicAdd(ROWS ? &s_row[wave][1] : &s_cnt[tg * 3 + 1], 1u);
        if (e & 2) atomicAdd(ROWS ? &s_row[wave][0] : &s_cnt[tp * 3 + 0], 1u);
        if (e == 3 && tg == tp) {
          const int bg = ent_prev(bits[ENT_START], c, true), bp = ent_prev(bits[ENT_START + 1], c, true);
          if (bg >= 0 && bg == bp) atomicAdd(ROWS ? &s_row[wave][2] : &s_cnt[tg * 3 + 2], 1u);
        }
      }
    }
    __syncthreads();  // the next sentence overwrites labels and words
    if (ROWS && active && lane < 3) rows_out[(long)row * 3 + lane] = (int32_t)s_row[wave][lane];
  }

  if (ROWS) return;
  for (int i = tid; i < n_cnt; i += 64 * ENT_WAVES) {
    const unsigned v = s_cnt[i];
    if (v) atomicAdd(&counts[i], (unsigned long long)v);
  }
}

}  // namespace mtvaf

using namespace mtvaf;

extern "C" {

int mtvaf_entity_counts(const int* pred, int ldp, const int64_t* gold, const uint8_t* mask, const uint8_t* start_tab,
                        const uint8_t* end_tab, const int* type_of, const uint8_t* gold_skip, int B, int S, int C,
                        int n_types, int64_t* counts, hipStream_t st) {
  if (B <= 0 || S < 1 || S > ENT_MAX_S || C < 1 || C > ENT_MAX_C || ldp < S) return MTVAF_ERR_SHAPE;
  if (n_types < 1 || n_types > C + 1) return MTVAF_ERR_ARG;
  if ((long)B * S > 0x7fffffffL) return MTVAF_ERR_SHAPE;  // a block's LDS counters are 32-bit
  const int blocks = min((B + ENT_WAVES - 1) / ENT_WAVES, 1024);
  hipLaunchKernelGGL(entity_counts_kernel<false>, dim3(blocks), dim3(64 * ENT_WAVES), 0, st, pred, ldp, gold, mask, start_tab,
                     end_tab, type_of, gold_skip, B, S, C, n_types, (unsigned long long*)counts, 1, nullptr);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

int mtvaf_entity_counts_rows(const int* pred, int ldp, int group, const int64_t* gold, const uint8_t* mask,
                             const uint8_t* start_tab, const uint8_t* end_tab, const int* type_of, const uint8_t* gold_skip,
                             int R, int S, int C, int n_types, int32_t* rows_out, hipStream_t st) {
  if (R <= 0 || S < 1 || S > ENT_MAX_S || C < 1 || C > ENT_MAX_C || ldp < S || group < 1 || R % group != 0)
    return MTVAF_ERR_SHAPE;
  if (n_types < 1 || n_types > C + 1) return MTVAF_ERR_ARG;
  if ((long)R * S > 0x7fffffffL) return MTVAF_ERR_SHAPE;
  const int blocks = min((R + ENT_WAVES - 1) / ENT_WAVES, 1024);
  hipLaunchKernelGGL(entity_counts_kernel<true>, dim3(blocks), dim3(64 * ENT_WAVES), 0, st, pred, ldp, gold, mask, start_tab,
                     end_tab, type_of, gold_skip, R, S, C, n_types, nullptr, group, rows_out);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

}  // extern "C"
