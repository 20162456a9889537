// Fused prefix self-attention for gfx950 (fp32, v_mfma_f32_16x16x4_f32):
//   K3/K4  softmax(Q.[Kp;K]^T / sqrt(D) + mask) . [Vp;V]  with the visual prefix K/V slab in FRONT of the
//          text keys, attention-prob dropout and head merge -- models/modeling_bert.py:282-286, 303,
//          320-337 (identical in models/modeling_roberta.py:218-222).
// The [B,NH,S,T] score/probability tensors of the reference are never materialised: the forward keeps
// a flash-style running (max, sum) per query and saves only the log-sum-exp; the backward recomputes
// the probabilities from it.
//
// Data layout (all fp32):
//   qkv   [B*S, 3H]  token-major output of the fused QKV projection (Q | K | V column blocks)
//   pk,pv [B, P*H]   one layer's prefix slab; head h, slot p, dim d at h*(P*64) + p*64 + d  -- the raw
//                    reshape(bsz, 12, -1, 64) of models/bert_model.py:585
//   addmask [B, T]   additive mask, T = P + S: (1 - mask) * -10000  (models/modeling_bert.py:1134-1137)
//   ctx   [B*S, H]   merged heads (modeling_bert.py:335-337)
//
// MFMA mapping: scores are produced TRANSPOSED (S^T[key][q] = K.Q^T) so that a query lives on a lane:
// softmax statistics are lane-local plus two shuffles, and the probability registers are directly
// the B operand of the P.V product (O^T[d][q] = V^T.P^T) -- no LDS round trip for P.  The k index of
// every product is permuted (step t, lane group g <-> k = 4g + t) identically on both operands.
//
// The kernel bodies are those of csrc/attention_skeleton.h; this file provides their fp32-pipe arithmetic and the C entry points.
#include "attention_skeleton.h"

namespace mtvaf {

#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// The fp32-pipe arithmetic: [64][64] fp32 tiles, padded rows; the operand of a row is its 64 values, 4 consecutive d per lane at
// 16 db + 4 g .. + 3 (db = 0 .. 3); every product is 16 v_mfma_f32_16x16x4_f32 over d (or over the 16 rows of a block).
struct PipeF32 : F32Io {
  typedef float Lds;
  static constexpr int LDT = 68;  // LDS row stride (floats) of a tile that is also read by columns: conflict-free b32 column reads
  static constexpr int LDK = 72;  // ... of a tile read as row fragments only: conflict-free ds_read_b128 (slot = 2*row + k-chunk mod 16)
  template <int LD>
  struct Tile {
    float* p;
  };
  typedef Tile<LDK> RowTile;
  typedef Tile<LDT> ColTile;

  // staging: thread -> rows r, r + 16, r + 32, r + 48 (r = tid >> 4), the 4 values at column 4 (tid & 15)
  static __device__ __forceinline__ int stage_col() { return (threadIdx.x & 15) * 4; }
  static __device__ __forceinline__ int operand_col(int g) { return 4 * g; }
  struct Stage {
    f32x4 v[4];
  };
  // Branch-free staging of the [prefix ; text] key axis: rows beyond T re-read row T-1 (finite values; their probabilities are
  // exactly 0 through the -1e30 entry of the mask tile); all loads of a tile are issued before the first LDS store.
  static __device__ __forceinline__ void fetch_kv(Stage& s, const KvSrc& src, int P, int T, int ld_txt, int t0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = (threadIdx.x >> 4) + 16 * i;
      s.v[i] = *reinterpret_cast<const f32x4*>(kv_row_ptr(src, min(t0 + r, T - 1), P, ld_txt));
    }
  }
  // rows q0 + r (clamped to n - 1) of Q (row stride 3 H), dO and O (row stride H)
  static __device__ __forceinline__ void fetch_rows(Stage& q, Stage& d, Stage& o, const float* qsrc, const float* dsrc, const float* osrc, int H,
                                                    int q0, int n) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int qq = min(q0 + (int)(threadIdx.x >> 4) + 16 * i, n - 1);
      q.v[i] = *reinterpret_cast<const f32x4*>(qsrc + (long)qq * 3 * H);
      d.v[i] = *reinterpret_cast<const f32x4*>(dsrc + (long)qq * H);
      o.v[i] = *reinterpret_cast<const f32x4*>(osrc + (long)qq * H);
    }
  }
  template <int LD>
  static __device__ __forceinline__ void store(Tile<LD> t, const Stage& s) {
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(t.p + ((threadIdx.x >> 4) + 16 * i) * LD + (threadIdx.x & 15) * 4) = s.v[i];
  }
  struct StageDelta {
    float s[4];
    __device__ __forceinline__ void reduce(const Stage& o, const Stage& d) {
#pragma unroll
      for (int i = 0; i < 4; ++i) s[i] = o.v[i].x * d.v[i].x + o.v[i].y * d.v[i].y + o.v[i].z * d.v[i].z + o.v[i].w * d.v[i].w;
#pragma unroll
      for (int i = 0; i < 4; ++i) {  // the 16 threads of a row are 16 consecutive lanes
        s[i] += __shfl_xor(s[i], 1, 64);
        s[i] += __shfl_xor(s[i], 2, 64);
        s[i] += __shfl_xor(s[i], 4, 64);
        s[i] += __shfl_xor(s[i], 8, 64);
      }
    }
    __device__ __forceinline__ void store(float* del_s) const {
      if ((threadIdx.x & 15) == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) del_s[(threadIdx.x >> 4) + 16 * i] = s[i];
      }
    }
  };

  struct Operand {
    f32x4 v[4];
  };
  static __device__ __forceinline__ Operand load_operand(const float* p) {
    Operand x;
#pragma unroll
    for (int db = 0; db < 4; ++db) x.v[db] = *reinterpret_cast<const f32x4*>(p + 16 * db);
    return x;
  }
  static __device__ __forceinline__ Operand load_operand_dot(const float* p, const float* op, float& dot) {
    Operand x;
#pragma unroll
    for (int db = 0; db < 4; ++db) {
      x.v[db] = *reinterpret_cast<const f32x4*>(p + 16 * db);
      const f32x4 o = *reinterpret_cast<const f32x4*>(op + 16 * db);
      dot += o.x * x.v[db].x + o.y * x.v[db].y + o.z * x.v[db].z + o.w * x.v[db].w;
    }
    return x;
  }

  // The k index of every product is permuted (step t, lane group g <-> k = 4g + t) identically on both operands.
  template <int LD>
  static __device__ __forceinline__ f32x4 rows_dot(Tile<LD> tile, int blk, const Operand& x, int lr, int g) {
    const float* frag = tile.p + (16 * blk + lr) * LD + 4 * g;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int db = 0; db < 4; ++db) {
      const f32x4 f = *reinterpret_cast<const f32x4*>(frag + 16 * db);
#pragma unroll
      for (int t = 0; t < 4; ++t) acc = MFMA16(f[t], x.v[db][t], acc);
    }
    return acc;
  }
  // (two independent accumulation chains, interleaved: a lone chain of 16 dependent MFMAs waits for every result)
  template <int LD0, int LD1>
  static __device__ __forceinline__ void rows_dot2(Tile<LD0> tile0, const Operand& x0, f32x4& r0, Tile<LD1> tile1, const Operand& x1, f32x4& r1,
                                                   int blk, int lr, int g) {
    const float* frag0 = tile0.p + (16 * blk + lr) * LD0 + 4 * g;
    const float* frag1 = tile1.p + (16 * blk + lr) * LD1 + 4 * g;
    r0 = r1 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int db = 0; db < 4; ++db) {
      const f32x4 f0 = *reinterpret_cast<const f32x4*>(frag0 + 16 * db);
      const f32x4 f1 = *reinterpret_cast<const f32x4*>(frag1 + 16 * db);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        r0 = MFMA16(f0[t], x0.v[db][t], r0);
        r1 = MFMA16(f1[t], x1.v[db][t], r1);
      }
    }
  }
  // One 16-row block at a time: its probability registers are directly the B operand, and the backward loops (168 VGPRs at three
  // waves per SIMD) cannot hold the dS of a whole tile.
  static constexpr int FOLD = 1;
  static __device__ __forceinline__ void cols_acc(ColTile tile, int j, const f32x4* p, int nsub, int lane, f32x4 (&acc)[4]) {
    const float* col = tile.p + 4 * (lane >> 4) * LDT + (lane & 15);
    if (j < nsub) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const float* row = col + (16 * j + t) * LDT;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) acc[dt] = MFMA16(row[16 * dt], p[0][t], acc[dt]);
      }
    }
  }

  // (the two accumulations of the key side, interleaved like the row products above and for the same reason: with the S / dP and the
  // dV / dK chains issued one behind the other the backward kernel measured 3 - 5 % slower)
  static __device__ __forceinline__ void cols_acc2(ColTile tile0, const f32x4* p0, f32x4 (&acc0)[4], ColTile tile1, const f32x4* p1,
                                                   f32x4 (&acc1)[4], int j, int nsub, int lane) {
    const float* col0 = tile0.p + 4 * (lane >> 4) * LDT + (lane & 15);
    const float* col1 = tile1.p + 4 * (lane >> 4) * LDT + (lane & 15);
    if (j < nsub) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const float* row0 = col0 + (16 * j + t) * LDT;
        const float* row1 = col1 + (16 * j + t) * LDT;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          acc0[dt] = MFMA16(row0[16 * dt], p0[0][t], acc0[dt]);
          acc1[dt] = MFMA16(row1[16 * dt], p1[0][t], acc1[dt]);
        }
      }
    }
  }

  // A query tile whose upstream gradient is all zeros (padded positions: nothing downstream reads them) has dP = dO.V^T = 0
  // and delta = 0, hence dS = 0 and dQ = 0 EXACTLY.  Detected, not assumed: one LDS flag (Ms[0] is free until the first key
  // tile is staged), no vote primitive.  (The same test on the key side -- skipping all-zero query tiles in the dK / dV loop --
  // measured 3 % SLOWER on the whole step, with a vote primitive and with plain LDS flags alike: the loop is at its register
  // limit.  The split arithmetic does not make the test at all.)
  static __device__ __forceinline__ bool tile_without_gradient(const Operand& dO, bool qok, float* Ms) {
    bool nz = false;
#pragma unroll
    for (int db = 0; db < 4; ++db) nz = nz || dO.v[db].x != 0.f || dO.v[db].y != 0.f || dO.v[db].z != 0.f || dO.v[db].w != 0.f;
    int* flag = reinterpret_cast<int*>(Ms);
    if (threadIdx.x == 0) *flag = 0;
    __syncthreads();
    if (qok && nz) *flag = 1;  // (benign race: every writer stores the same value)
    __syncthreads();
    const bool live = *flag != 0;
    __syncthreads();  // (the flag word is the mask tile's first entry: nobody may still read it when staging starts)
    return !live;
  }
};

__global__ __launch_bounds__(256) void attn_fwd_kernel(AttnArgs a) {
  __shared__ __attribute__((aligned(16))) float Ks[KT * PipeF32::LDK];
  __shared__ __attribute__((aligned(16))) float Vs[KT * PipeF32::LDT];
  __shared__ __attribute__((aligned(16))) float Ms[KT];
  __shared__ int t_eff_slot;
  attn_fwd_body<PipeF32>(a, PipeF32::RowTile{Ks}, PipeF32::ColTile{Vs}, Ms, &t_eff_slot);
}

// (the forward's LDS with the transposing buffer in the place of the V tile)
__global__ __launch_bounds__(256) void attn_probs_kernel(AttnArgs a, ProbsOut o) {
  __shared__ __attribute__((aligned(16))) float Ks[KT * PipeF32::LDK];
  __shared__ __attribute__((aligned(16))) float Ps[KT * LDP];
  __shared__ __attribute__((aligned(16))) float Ms[KT];
  __shared__ int t_eff_slot;
  attn_probs_body<PipeF32>(a, o, PipeF32::RowTile{Ks}, Ps, Ms, &t_eff_slot);
}

// (each side of the backward is VALU / issue bound at ~40 % MFMA utilisation on its own)
__global__ __launch_bounds__(256, 3) void attn_bwd_kernel(AttnArgs a, int nq) {  // 4 per SIMD spills 10 VGPRs
  __shared__ __attribute__((aligned(16))) float tile0[KT * PipeF32::LDK];
  __shared__ __attribute__((aligned(16))) float tile1[KT * PipeF32::LDK];
  __shared__ __attribute__((aligned(16))) float small[3 * KT];
  __shared__ int t_eff_slot;
  attn_bwd_body<PipeF32>(a, nq, tile0, tile1, small, nullptr, &t_eff_slot);
}

// The packed-row kernels with a per-sentence prefix-slot mask (mask_at<PM>): the same bodies, LDS and launch bounds; pmask is an
// argument of its own, so the kernels above keep their argument block and their code.
__global__ __launch_bounds__(256) void attn_fwd_pm_kernel(AttnArgs a, const float* pmask) {
  __shared__ __attribute__((aligned(16))) float Ks[KT * PipeF32::LDK];
  __shared__ __attribute__((aligned(16))) float Vs[KT * PipeF32::LDT];
  __shared__ __attribute__((aligned(16))) float Ms[KT];
  __shared__ int t_eff_slot;
  attn_fwd_body<PipeF32, true>(a, PipeF32::RowTile{Ks}, PipeF32::ColTile{Vs}, Ms, &t_eff_slot, pmask);
}

__global__ __launch_bounds__(256, 3) void attn_bwd_pm_kernel(AttnArgs a, int nq, const float* pmask) {
  __shared__ __attribute__((aligned(16))) float tile0[KT * PipeF32::LDK];
  __shared__ __attribute__((aligned(16))) float tile1[KT * PipeF32::LDK];
  __shared__ __attribute__((aligned(16))) float small[3 * KT];
  __shared__ int t_eff_slot;
  attn_bwd_body<PipeF32, true>(a, nq, tile0, tile1, small, nullptr, &t_eff_slot, pmask);
}

}  // namespace mtvaf

using namespace mtvaf;

extern "C" {

// Round 6: under the split arithmetic (the library default: mtvaf_f32_split) the attention products are split bf16 products too
// (csrc/attention_f32s.hip: same interface, geometry and outputs); the fp32 MFMA pipe keeps the kernels of this file.
static bool attn_split_on() { return mtvaf_f32_split(-1) != 0; }

static int attn_fwd_launch(const float* qkv, const float* pk, const float* pv, const float* addmask, const int* cu, int pad_rows,
                           float* ctx, float* lse, int B, int S, int P, int NH, int head_dim, float p_drop, uint64_t seed,
                           uint64_t offset, hipStream_t st, void* ctx_planes = nullptr, long rows = 0, const float* pmask = nullptr) {
  if (head_dim != D) return MTVAF_ERR_SHAPE;
  if (!cu && !addmask) return MTVAF_ERR_ARG;
  AttnArgs a{};
  a.qkv = qkv; a.pk = pk; a.pv = pv; a.addmask = addmask; a.cu = cu; a.pad_rows = pad_rows; a.ctx = ctx; a.lse = lse;
  a.ctx_p = static_cast<unsigned char*>(ctx_planes); a.Mrows = rows;
  if (ctx_planes && (!cu || rows <= 0 || (((uintptr_t)ctx_planes) & 15))) return MTVAF_ERR_ARG;
  attn_fill_common(a, B, S, P, NH, p_drop, seed, offset);
  int rc = attn_check(a);
  if (rc) return rc;
  if (pad_rows < 0 || (pad_rows && !cu)) return MTVAF_ERR_ARG;
  const dim3 grid((S + 63) / 64, NH, B + (pad_rows > 0 ? 1 : 0));
  if (attn_split_on()) return launch_attn_f32s_fwd(a, grid, st, pmask);
  if (pmask) hipLaunchKernelGGL(attn_fwd_pm_kernel, grid, dim3(256), 0, st, a, pmask);
  else hipLaunchKernelGGL(attn_fwd_kernel, grid, dim3(256), 0, st, a);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

static int attn_bwd_launch(const float* dctx, const float* qkv, const float* pk, const float* pv, const float* addmask,
                           const int* cu, int pad_rows, const float* ctx, const float* lse, float* delta, float* dqkv, float* dpk, float* dpv,
                           int B, int S, int P, int NH, int head_dim, float p_drop, uint64_t seed, uint64_t offset, hipStream_t st,
                           int zero_tail = 0, void* dqkv_planes = nullptr, long rows = 0, const float* pmask = nullptr) {
  if (head_dim != D) return MTVAF_ERR_SHAPE;
  if (!cu && !addmask) return MTVAF_ERR_ARG;
  AttnArgs a{};
  a.qkv = qkv; a.pk = pk; a.pv = pv; a.addmask = addmask; a.cu = cu; a.pad_rows = pad_rows; a.ctx = const_cast<float*>(ctx);
  a.lse = const_cast<float*>(lse); a.dctx = dctx; a.delta = delta; a.dqkv = dqkv; a.dpk = dpk; a.dpv = dpv;
  a.zero_tail = zero_tail;
  a.dqkv_p = static_cast<unsigned char*>(dqkv_planes); a.Mrows = rows;
  if (dqkv_planes && (!cu || rows <= 0 || (((uintptr_t)dqkv_planes) & 15))) return MTVAF_ERR_ARG;
  attn_fill_common(a, B, S, P, NH, p_drop, seed, offset);
  int rc = attn_check(a);
  if (rc) return rc;
  if (P > 0 && (!dpk || !dpv)) return MTVAF_ERR_ARG;
  if (pad_rows < 0 || (pad_rows && !cu)) return MTVAF_ERR_ARG;
  const int nq = (S + 63) / 64;
  const dim3 grid(nq + (P + S + 63) / 64, NH, B + (pad_rows > 0 ? 1 : 0));
  if (attn_split_on()) return launch_attn_f32s_bwd(a, nq, grid, st, pmask);
  if (pmask) hipLaunchKernelGGL(attn_bwd_pm_kernel, grid, dim3(256), 0, st, a, nq, pmask);
  else hipLaunchKernelGGL(attn_bwd_kernel, grid, dim3(256), 0, st, a, nq);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

static int attn_probs_launch(const float* qkv, const float* pk, const float* addmask, float* probs, float* prefix_mass, int B, int S,
                             int P, int NH, int head_dim, int zero_masked_queries, hipStream_t st) {
  if (head_dim != D) return MTVAF_ERR_SHAPE;
  if (!qkv || !addmask) return MTVAF_ERR_ARG;
  AttnArgs a{};
  a.qkv = qkv; a.pk = pk; a.pv = pk; a.addmask = addmask;  // (no V: the value sources are never read)
  attn_fill_common(a, B, S, P, NH, 0.f, 0, 0);
  int rc = attn_check(a);
  if (rc) return rc;
  const ProbsOut o{probs, prefix_mass, zero_masked_queries};
  const dim3 grid((S + 63) / 64, NH, B);
  if (attn_split_on()) return launch_attn_f32s_probs(a, o, grid, st);
  hipLaunchKernelGGL(attn_probs_kernel, grid, dim3(256), 0, st, a, o);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

// probs[B,NH,S,P+S] (every element written), prefix_mass[B,NH,S] (or NULL) <- softmax(Q.[Kp;K]^T / sqrt(D) + addmask): the
// probabilities the forward never materialises, by the arithmetic it runs with (mtvaf_f32_split).  Only the Q and K thirds of qkv
// are read.
int mtvaf_prefix_attn_probs(const float* qkv, const float* pk, const float* addmask, float* probs, float* prefix_mass, int B, int S,
                            int P, int NH, int head_dim, int zero_masked_queries, hipStream_t st) {
  if (!probs) return MTVAF_ERR_ARG;
  return attn_probs_launch(qkv, pk, addmask, probs, prefix_mass, B, S, P, NH, head_dim, zero_masked_queries, st);
}

// prefix_mass alone: the same kernel without the [B,NH,S,P+S] stores (its second pass ends behind the prefix slots).
int mtvaf_prefix_attn_mass(const float* qkv, const float* pk, const float* addmask, float* prefix_mass, int B, int S, int P, int NH,
                           int head_dim, int zero_masked_queries, hipStream_t st) {
  if (!prefix_mass) return MTVAF_ERR_ARG;
  return attn_probs_launch(qkv, pk, addmask, nullptr, prefix_mass, B, S, P, NH, head_dim, zero_masked_queries, st);
}

// ctx[B*S,H], lse[B,NH,S] <- attention over [prefix ; text] keys.  head_dim must be 64.
int mtvaf_prefix_attn_fwd(const float* qkv, const float* pk, const float* pv, const float* addmask, float* ctx,
                          float* lse, int B, int S, int P, int NH, int head_dim, float p_drop, uint64_t seed,
                          uint64_t offset, hipStream_t st) {
  return attn_fwd_launch(qkv, pk, pv, addmask, nullptr, 0, ctx, lse, B, S, P, NH, head_dim, p_drop, seed, offset, st);
}

// dqkv[B*S,3H] (all three column blocks overwritten), dpk/dpv[B,P*H] <- gradients; delta[B,NH,S] scratch.
int mtvaf_prefix_attn_bwd(const float* dctx, const float* qkv, const float* pk, const float* pv,
                          const float* addmask, const float* ctx, const float* lse, float* delta, float* dqkv,
                          float* dpk, float* dpv, int B, int S, int P, int NH, int head_dim, float p_drop,
                          uint64_t seed, uint64_t offset, hipStream_t st) {
  return attn_bwd_launch(dctx, qkv, pk, pv, addmask, nullptr, 0, ctx, lse, delta, dqkv, dpk, dpv, B, S, P, NH, head_dim, p_drop, seed,
                         offset, st);
}

// mtvaf_prefix_attn_bwd for callers that vouch that dctx is exactly zero for the queries behind a sentence's last unmasked text
// position (zero_tail != 0; see AttnArgs): same results bit for bit under that contract, the query loops stop there.
int mtvaf_prefix_attn_bwd_tail(const float* dctx, const float* qkv, const float* pk, const float* pv, const float* addmask,
                               const float* ctx, const float* lse, float* delta, float* dqkv, float* dpk, float* dpv, int B, int S,
                               int P, int NH, int head_dim, float p_drop, uint64_t seed, uint64_t offset, int zero_tail,
                               hipStream_t st) {
  return attn_bwd_launch(dctx, qkv, pk, pv, addmask, nullptr, 0, ctx, lse, delta, dqkv, dpk, dpv, B, S, P, NH, head_dim, p_drop, seed,
                         offset, st, zero_tail);
}

// The same attention over PACKED token rows (padding-free execution): cu [B+1] int32 row offsets -- sentence b owns rows
// cu[b] .. cu[b+1]-1 of qkv / ctx / dctx / dqkv (its unmasked tokens, at most S of them).  Every kept key is unmasked, so
// no additive mask is read; lse / delta stay [B,NH,S].  The pad_rows rows behind the last sentence (they pad the packed
// image to whole tiles) are zero-filled in ctx / dqkv by an extra slice of the same launch.
int mtvaf_prefix_attn_varlen_fwd(const float* qkv, const float* pk, const float* pv, const int* cu, int pad_rows, float* ctx,
                                 float* lse, int B, int S, int P, int NH, int head_dim, float p_drop, uint64_t seed, uint64_t offset,
                                 hipStream_t st) {
  if (!cu) return MTVAF_ERR_ARG;
  return attn_fwd_launch(qkv, pk, pv, nullptr, cu, pad_rows, ctx, lse, B, S, P, NH, head_dim, p_drop, seed, offset, st);
}

int mtvaf_prefix_attn_varlen_bwd(const float* dctx, const float* qkv, const float* pk, const float* pv, const int* cu, int pad_rows,
                                 const float* ctx, const float* lse, float* delta, float* dqkv, float* dpk, float* dpv, int B, int S,
                                 int P, int NH, int head_dim, float p_drop, uint64_t seed, uint64_t offset, hipStream_t st) {
  if (!cu) return MTVAF_ERR_ARG;
  return attn_bwd_launch(dctx, qkv, pk, pv, nullptr, cu, pad_rows, ctx, lse, delta, dqkv, dpk, dpv, B, S, P, NH, head_dim, p_drop, seed,
                         offset, st);
}

// The packed-row attention that ALSO writes the tile-blocked plane image of its GEMM-operand result (round 5, pre-split operands:
// csrc/gemm_f32p.hip): the context as [H / 32][3][rows][32] -- the operand of the Wo product and of its weight gradient -- / dQ | dK |
// dV as [3H / 32][3][rows][32] -- the operand of the QKV dX product and of its weight gradient; rows = the packed image's row count
// (whole 128-row tiles).  Bit for bit what mtvaf_f32_split_planes writes over the fp32 result, which is written too.
int mtvaf_prefix_attn_varlen_fwd_planes(const float* qkv, const float* pk, const float* pv, const int* cu, int pad_rows, float* ctx,
                                        float* lse, int B, int S, int P, int NH, int head_dim, float p_drop, uint64_t seed,
                                        uint64_t offset, void* ctx_planes, int rows, hipStream_t st) {
  if (!cu || !ctx_planes) return MTVAF_ERR_ARG;
  return attn_fwd_launch(qkv, pk, pv, nullptr, cu, pad_rows, ctx, lse, B, S, P, NH, head_dim, p_drop, seed, offset, st, ctx_planes, rows);
}
int mtvaf_prefix_attn_varlen_bwd_planes(const float* dctx, const float* qkv, const float* pk, const float* pv, const int* cu, int pad_rows,
                                        const float* ctx, const float* lse, float* delta, float* dqkv, float* dpk, float* dpv, int B,
                                        int S, int P, int NH, int head_dim, float p_drop, uint64_t seed, uint64_t offset,
                                        void* dqkv_planes, int rows, hipStream_t st) {
  if (!cu || !dqkv_planes) return MTVAF_ERR_ARG;
  return attn_bwd_launch(dctx, qkv, pk, pv, nullptr, cu, pad_rows, ctx, lse, delta, dqkv, dpk, dpv, B, S, P, NH, head_dim, p_drop, seed,
                         offset, st, 0, dqkv_planes, rows);
}

// The packed-row attention with a per-sentence PREFIX-SLOT MASK: pmask [B, P] fp32 additive, 0 = sentence b owns the slot, -10000 =
// it does not -- the prefix columns of the padded layout's addmask, added at the same place of the arithmetic, so a packed run with
// a mask equals the padded run with the same mask to the degree the unmasked runs agree.  A masked slot has probability exactly 0
// (exp2 underflows as in the padded layout) and its rows of dpk / dpv are exactly 0; a sentence with every slot masked attends to
// its own text keys.  No tile is skipped: same products, same order, only the mask tile differs.  pmask_len = B * P, the element
// count of pmask (MTVAF_ERR_ARG otherwise, and for a pmask with P == 0).  pmask == NULL (pmask_len ignored): the launch of
// mtvaf_prefix_attn_varlen_fwd / _bwd, or of their _planes forms when ctx_planes / dqkv_planes is given (NULL: no plane image).
static int pmask_check(const float* pmask, long pmask_len, int B, int P) {
  if (!pmask) return MTVAF_OK;
  if (P <= 0 || B <= 0 || pmask_len != (long)B * P) return MTVAF_ERR_ARG;
  return MTVAF_OK;
}
int mtvaf_prefix_attn_varlen_fwd_pm(const float* qkv, const float* pk, const float* pv, const int* cu, int pad_rows,
                                    const float* pmask, long pmask_len, float* ctx, float* lse, int B, int S, int P, int NH,
                                    int head_dim, float p_drop, uint64_t seed, uint64_t offset, void* ctx_planes, int rows,
                                    hipStream_t st) {
  if (!cu) return MTVAF_ERR_ARG;
  if (int rc = pmask_check(pmask, pmask_len, B, P)) return rc;
  return attn_fwd_launch(qkv, pk, pv, nullptr, cu, pad_rows, ctx, lse, B, S, P, NH, head_dim, p_drop, seed, offset, st, ctx_planes,
                         ctx_planes ? rows : 0, pmask);
}
int mtvaf_prefix_attn_varlen_bwd_pm(const float* dctx, const float* qkv, const float* pk, const float* pv, const int* cu, int pad_rows,
                                    const float* pmask, long pmask_len, const float* ctx, const float* lse, float* delta, float* dqkv,
                                    float* dpk, float* dpv, int B, int S, int P, int NH, int head_dim, float p_drop, uint64_t seed,
                                    uint64_t offset, void* dqkv_planes, int rows, hipStream_t st) {
  if (!cu) return MTVAF_ERR_ARG;
  if (int rc = pmask_check(pmask, pmask_len, B, P)) return rc;
  return attn_bwd_launch(dctx, qkv, pk, pv, nullptr, cu, pad_rows, ctx, lse, delta, dqkv, dpk, dpv, B, S, P, NH, head_dim, p_drop, seed,
                         offset, st, 0, dqkv_planes, dqkv_planes ? rows : 0, pmask);
}

}  // extern "C"
