// Argument blocks of the prefix-attention kernels: AttnArgs of the two fp32 arithmetics -- csrc/attention.hip (fp32 MFMA pipe) and
// csrc/attention_f32s.hip (round 6: the same attention with its products formed as split bf16 products, the arithmetic of
// csrc/gemm_f32x3.hip) -- and ab::Args of the mixed-precision one (csrc/attention_bf16.hip): same launch geometry, same key order,
// same dropout hash in all three.  With them the stores of the results that are GEMM operands downstream (store_ctx / store_dqkv, one
// overload per block) and the small device / host helpers, written over any argument struct with cu, B, S, addmask.  The kernel
// bodies live once in csrc/attention_skeleton.h, templates over an arithmetic (element type and argument block, LDS tile format,
// staging registers, register operand, products, output hooks).
#pragma once
#include "common.h"
#include "planes.h"

namespace mtvaf {

constexpr int D = 64;      // head dim (asserted by the launcher)
constexpr int KT = 64;     // keys (or queries) per LDS tile
constexpr float NEG_BIG = -1.0e30f;
constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;

struct AttnArgs {
  const float* qkv;
  const float* pk;
  const float* pv;
  const float* addmask;
  float* ctx;
  float* lse;
  // backward
  const float* dctx;
  float* delta;
  float* dqkv;
  float* dpk;
  float* dpv;
  int B, S, P, NH, H;
  float scale, p_drop;
  uint32_t drop_key, drop_thr;
  const uint64_t* epoch;  // device-side dropout epoch (captured launches), or NULL
  // PACKED token rows (padding-free execution): sentence b owns rows cu[b] .. cu[b+1]-1 of qkv / ctx / dctx / dqkv (its
  // unmasked tokens, in order), every kept key is unmasked (addmask is not read), queries beyond the sentence do not
  // exist.  NULL: the padded [B, S] layout.  lse / delta / the dropout row ids keep the [B, NH, S] indexing either way.
  const int* cu;
  int pad_rows;  // packed rows: this many rows behind the last sentence pad the image; the z-slice b == B zero-fills them
  // backward, padded layout: the caller vouches that dctx is EXACTLY zero for the queries behind the last unmasked text position
  // of a sentence (trailing padding: nothing downstream reads those rows -- the contract of the k-tile lists of the weight
  // gradients).  Their dQ is exactly zero and they add exactly nothing to dK / dV: the key side stops its query loop there.
  int zero_tail;
  // pre-split operands (round 5; packed rows only): ALSO write the tile-blocked plane image of the context ([H / 32][3][Mrows][32])
  // / of dQ | dK | dV ([3H / 32][3][Mrows][32]) -- what the Wo / QKV-dX products and the weight gradients read -- or NULL
  unsigned char* ctx_p;
  unsigned char* dqkv_p;
  long Mrows;
};

namespace ab {

// The mixed-precision mode: Q | K | V, the prefix slabs, the context and their gradients are bf16 (no fp32 copies of these tensors
// exist), and the per-head column sums of dQ | dK | dV (the QKV bias gradient) leave the backward kernel as per-block partials.
struct Args {
  const __bf16* qkv;
  const __bf16* pk;
  const __bf16* pv;
  const float* addmask;
  __bf16* ctx;
  float* lse;
  // backward
  const __bf16* dctx;
  __bf16* dqkv;
  float* dpk;
  float* dpv;
  float* partq;   // [B * nqt][H]   column sums of dQ per query-tile block
  float* partkv;  // [B * nkt][2H]  column sums of dK | dV (text keys only) per key-tile block
  int B, S, P, NH, H;
  float scale, p_drop;
  uint32_t drop_key, drop_thr;
  const uint64_t* epoch;  // device-side dropout epoch (captured launches), or NULL
  const int* cu;          // PACKED token rows (see AttnArgs): [B+1] row offsets of the sentences, or NULL
  int pad_rows;           // rows behind the last sentence that pad the packed image: zero-filled by the z-slice b == B
  int zero_tail;          // backward, padded layout: dctx is exactly zero behind a sentence's last unmasked position (the caller's
                          // word, as AttnArgs::zero_tail): the key side's query loop stops there
};

}  // namespace ab

// outputs of the probabilities-on-request kernel (attn_probs_body): beside AttnArgs, so that the training kernels' argument block
// stays as it is
struct ProbsOut {
  float* probs;  // NULL: only mass is wanted -- the second pass stops behind the prefix slots
  float* mass;   // or NULL
  int zero_masked_queries;  // rows of queries whose own key is masked (addmask <= -5000): zeros
};

// the stores of the two results that are GEMM operands downstream: fp32, and the plane image when the caller asked for it
__device__ __forceinline__ void store_ctx(const AttnArgs& a, long row, int col, const f32x4 v) {
  *reinterpret_cast<f32x4*>(a.ctx + row * a.H + col) = v;
  if (a.ctx_p) planes_store4(a.ctx_p, a.Mrows, row, col, v);
}
__device__ __forceinline__ void store_dqkv(const AttnArgs& a, long row, int col, const f32x4 v) {
  *reinterpret_cast<f32x4*>(a.dqkv + row * 3 * a.H + col) = v;
  if (a.dqkv_p) planes_store4(a.dqkv_p, a.Mrows, row, col, v);
}

// ... of the mixed-precision mode: rounded to bf16, four values per store
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void store_ctx(const ab::Args& a, long row, int col, const f32x4 v) {
  *reinterpret_cast<bf16x4*>(a.ctx + row * a.H + col) = bf16x4{(__bf16)v.x, (__bf16)v.y, (__bf16)v.z, (__bf16)v.w};
}
__device__ __forceinline__ void store_dqkv(const ab::Args& a, long row, int col, const f32x4 v) {
  *reinterpret_cast<bf16x4*>(a.dqkv + row * 3 * a.H + col) = bf16x4{(__bf16)v.x, (__bf16)v.y, (__bf16)v.z, (__bf16)v.w};
}

struct Sent {
  long tok0;  // first token row of the sentence
  int n;      // its text tokens (queries; text keys)
};
template <class Args>
__device__ __forceinline__ Sent sentence(const Args& a, int b) {
  if (a.cu) {
    const int c0 = b ? a.cu[b] : 0;  // (cu[0] = -1 marks a launch order behind the offsets: slot_sentence)
    return Sent{(long)c0, a.cu[b + 1] - c0};
  }
  return Sent{(long)b * a.S, a.S};
}
// the sentence of grid slot z (mtvaf_build_packing_ordered: longest first; identity without the list)
template <class Args>
__device__ __forceinline__ int slot_sentence(const Args& a, int z) {
  return (a.cu && a.cu[0] < 0) ? a.cu[a.B + 1 + z] : z;
}
// Additive mask of key t of sentence b.  PM (the *_pm kernels: packed rows with a per-sentence prefix-slot mask): pmask [B, P] holds
// the prefix columns of the padded layout's addmask (0 = slot present, -10000 = absent), indexed by the SENTENCE (not the grid slot)
// and added at the same place of the arithmetic, so a masked slot's probability underflows to exactly 0 as it does there; the text
// keys of packed rows stay unmasked.  PM is a template parameter and pmask a kernel argument of its own: the kernels without a
// mask are the code they were, argument block included.
template <bool PM = false, class Args>
__device__ __forceinline__ float mask_at(const Args& a, int b, int Tf, int t, const float* pmask = nullptr) {
  if constexpr (PM) {
    if (a.cu) return t < a.P ? pmask[(long)b * a.P + t] : 0.f;
  }
  return a.cu ? 0.f : a.addmask[(long)b * Tf + t];
}

// Keys behind the LAST unmasked text position of a sentence (trailing padding: additive mask -10000) contribute exactly 0
// to every probability sum -- exp2 underflows to 0 -- and leave the running maximum untouched, so whole key tiles made of
// them can be skipped with bit-identical results.  -> T_eff = P + 1 + max{s : addmask[b][P+s] > -5000}; the full T when
// no text key is unmasked (nothing is skipped then).  Masked keys BEFORE that position ("holes") stay in the loop.
__device__ __forceinline__ int effective_keys(const float* __restrict__ addmask_row, int P, int S, int* lds_slot) {
  if (threadIdx.x == 0) *lds_slot = -1;
  __syncthreads();
  int last = -1;
  for (int t = threadIdx.x; t < S; t += blockDim.x)
    if (addmask_row[P + t] > -5000.f) last = t;
  if (last >= 0) atomicMax(lds_slot, last);
  __syncthreads();
  const int l = *lds_slot;
  return l >= 0 ? P + l + 1 : P + S;
}

// Branch-free staging of [64][64] tiles of the [prefix ; text] key axis: rows beyond T re-read row T-1 (finite
// values; their probabilities are exactly 0 through the -1e30 entry of the mask tile).  The source pointer is
// selected with bit arithmetic (a ternary on pointers compiles to divergent branches whose loads the compiler
// then serialises with vmcnt(0) waits), and all loads of a tile are issued before the first LDS store.
template <class T>
struct KvSrcT {
  const T* pre;  // prefix slab of this (b, h), + the thread's column offset
  const T* txt;  // text rows of this (b, h), + the thread's column offset
};
typedef KvSrcT<float> KvSrc;
template <class T>
__device__ __forceinline__ const T* kv_row_ptr(const KvSrcT<T>& s, int t, int P, int ld_txt) {
  const bool ispre = t < P;
  const uint64_t m = ispre ? ~0ull : 0ull;
  const uint64_t base = (uint64_t)s.txt ^ (((uint64_t)s.txt ^ (uint64_t)s.pre) & m);
  const int off = ispre ? t * D : (t - P) * ld_txt;
  return reinterpret_cast<const T*>(base) + off;
}
// byte offset of 16-byte chunk c (0..7) of row r in a [64][64] bf16 tile image (128-byte rows): conflict-free for the row reads
// (ds_read_b128) and for the transposing reads (ds_read_b64_tr_b16) alike
__device__ __forceinline__ int tile_off(int r, int c) { return r * 128 + ((c ^ (((r >> 1) & 3) << 1)) << 4); }

// XCD-aware block order (round 5).  Workgroups are dealt round-robin over the 8 XCDs by their linear id, x fastest: the nx blocks
// of one (sentence, head) -- 2 query tiles forward; 2 query + 3 key tiles backward, which all read the same q / k / v / dO / O
// slices (3.5x the unique bytes: 165 - 205 MB per backward launch by the PMC counters against ~50 MB) -- landed on nx different
// XCDs, each with a private L2.  This bijective remap gives the k-th group of nx consecutive slots of ONE XCD to one
// (sentence, head), so the re-reads hit that XCD's L2.  Placement is a speed hint only: results never depend on it.
// Identity when the number of (sentence, head) pairs is not a multiple of 8.  nz = the sentences (the zero-fill slice z == B of a
// packed launch is dispatched behind them and keeps its index).
#ifndef MTVAF_ATTN_XCD_GROUP
#define MTVAF_ATTN_XCD_GROUP 1
#endif
__device__ __forceinline__ void xcd_group(int nx, int ny, int nz, int& x, int& y, int& z) {
  if (!MTVAF_ATTN_XCD_GROUP || ((ny * nz) & 7) || z >= nz) return;
  const int L = x + nx * (y + ny * z);
  const int xcd = L & 7, slot = L >> 3;
  const int gi = (slot / nx) * 8 + xcd;
  x = slot % nx;
  y = gi % ny;
  z = gi / ny;
}

// host side: the dropout key (replica of attn_dropout_key) and keep threshold of a launch; the fields that every launcher fills in
// and the tests it makes first
inline uint32_t attn_drop_key(uint64_t seed, uint64_t offset) {
  auto mix = [](uint32_t x) { x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16; return x; };
  return mix((uint32_t)seed ^ mix((uint32_t)(seed >> 32) ^ mix((uint32_t)offset ^ 0x9E3779B9u)));
}
inline uint32_t attn_drop_thr(float p_drop) { return p_drop > 0.f ? (uint32_t)fminf(p_drop * 4294967296.0f, 4294967040.0f) : 0u; }
template <class Args>
void attn_fill_common(Args& a, int B, int S, int P, int NH, float p_drop, uint64_t seed, uint64_t offset) {
  a.B = B; a.S = S; a.P = P; a.NH = NH; a.H = NH * D;
  a.scale = 0.125f; a.p_drop = p_drop;
  a.drop_thr = attn_drop_thr(p_drop);
  a.drop_key = attn_drop_key(seed, offset);
  a.epoch = rng_epoch_ptr();
}
template <class Args>
int attn_check(const Args& a) {
  if (a.B <= 0 || a.S <= 0 || a.P < 0 || a.NH <= 0 || a.H != a.NH * D) return MTVAF_ERR_SHAPE;
  if ((long)a.B * a.NH * a.S >= (1L << 32)) return MTVAF_ERR_SHAPE;
  if (a.p_drop < 0.f || a.p_drop >= 1.f) return MTVAF_ERR_ARG;
  if (a.P > 0 && (!a.pk || !a.pv)) return MTVAF_ERR_ARG;
  return MTVAF_OK;
}

// launchers of the split-product kernels (csrc/attention_f32s.hip); grid / block as the fp32-pipe kernels of attention.hip
// (pmask: the per-sentence prefix-slot mask of a packed launch, mask_at<PM>; NULL: the kernels without one)
int launch_attn_f32s_fwd(const AttnArgs& a, dim3 grid, hipStream_t st, const float* pmask = nullptr);
int launch_attn_f32s_bwd(const AttnArgs& a, int nq, dim3 grid, hipStream_t st, const float* pmask = nullptr);
int launch_attn_f32s_probs(const AttnArgs& a, const ProbsOut& o, dim3 grid, hipStream_t st);

}  // namespace mtvaf
