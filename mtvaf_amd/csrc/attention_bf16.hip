// Fused prefix self-attention of the mixed-precision mode (bf16 operands, v_mfma_f32_16x16x32_bf16, fp32 softmax
// statistics and accumulation): the same algorithm, key order, masking and dropout hash as attention.hip
//   softmax(Q.[Kp;K]^T / sqrt(D) + mask) . [Vp;V]     models/modeling_bert.py:282-286, 303, 320-337
// reading the bf16 Q|K|V written by the QKV projection's epilogue and writing the bf16 context / bf16 dQ|dK|dV that the
// next projections consume -- no fp32 copies of these tensors exist in this mode, and the per-head column sums of
// dQ|dK|dV (the QKV bias gradient) leave the backward kernel as per-block partials.
//
// Data layout:
//   qkv16   [B*S, 3H] bf16  token-major (Q | K | V column blocks)
//   pk16,pv16 [B, P*H] bf16 one layer's prefix slab (head h, slot p, dim d at h*(P*64) + p*64 + d), cast once per step
//   addmask [B, T] fp32     additive mask, T = P + S
//   ctx16   [B*S, H] bf16   merged heads;  lse [B, NH, S] fp32 (natural log)
//
// MFMA mapping (as attention.hip, 8x the k-depth): scores are produced TRANSPOSED, S^T[key][q] = K.Q^T, so a query
// lives on a lane (A = K rows from LDS by ds_read_b128, B = Q straight from global memory: 8 consecutive d per lane);
// the C layout hands lane (q, g) the keys 16*kb + 4g + r, which -- rounded to bf16 -- ARE the B operand of
// O^T[d][q] = V^T.P^T when the k-slot (g, j) of that product is defined as key 16*(2u + (j >> 2)) + 4g + (j & 3); the
// matching A operand V^T comes from the row-major V tile by two transposing reads (ds_read_b64_tr_b16).  All [64][64]
// bf16 tiles (128-byte rows) use ONE LDS image that is conflict-free for both the row reads and the transposing reads:
// 16-byte chunk c of row r at chunk c ^ (((r >> 1) & 3) << 1)  (tile_off, attention_args.h).
//
// The kernel bodies are those of csrc/attention_skeleton.h; this file provides their bf16 arithmetic (ab::Bf16), whose output hooks
// reduce the bias-gradient partials, and the C entry points.
#include "attention_skeleton.h"

namespace mtvaf {

namespace ab {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

#define MFMA_BF(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16((a), (b), (c), 0, 0, 0)

// A operand of a "rows x d" product: row (16*blk + lane&15), the 8 d values 32*ks + 8g .. +7
__device__ __forceinline__ bf16x8 row_frag(const unsigned char* tile, int blk, int ks, int lr, int g) {
  return *reinterpret_cast<const bf16x8*>(tile + tile_off(16 * blk + lr, 4 * ks + g));
}
// A operand of a "d x rows" product (transposed read): d = 16*dt + lane&15, k-slot (g, j) = tile row
// 16*(2u + (j >> 2)) + 4g + (j & 3).  Lane 4q+p of a 16-lane group addresses row q, columns 4p..4p+3 of the 4 x 16 block.
__device__ __forceinline__ bf16x8 tr_frag(const unsigned char* tile, int u, int dt, int lane) {
  const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
  const int r0 = 32 * u + 4 * g + q, r1 = r0 + 16;
  const int c = 2 * dt + (p >> 1), e = 8 * (p & 1);
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(tile + tile_off(r0, c) + e));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(tile + tile_off(r1, c) + e));
  return __builtin_bit_cast(bf16x8, (s16x8)__builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}
__device__ __forceinline__ bf16x8 pack8(const f32x4& a, const f32x4& b) {
  return bf16x8{(__bf16)a.x, (__bf16)a.y, (__bf16)a.z, (__bf16)a.w, (__bf16)b.x, (__bf16)b.y, (__bf16)b.z, (__bf16)b.w};
}
__device__ __forceinline__ float dot8(const bf16x8& a, const bf16x8& b) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) s += (float)a[i] * (float)b[i];
  return s;
}

// The bf16 arithmetic: a tile is one [64][64] bf16 image; the operand of a row is its 64 values, 8 consecutive d per lane at
// 32 ks + 8 g .. + 7 (ks = 0, 1); a product over d is two bf16 MFMA products, a product over a tile's rows two per 16 d.
struct Bf16 {
  typedef __bf16 Elem;
  typedef ab::Args Args;
  // (prefetching the next key tile into registers, as the backward does, measured 6 % SLOWER in the forward: 13.6 -> 14.5 us)
  static constexpr bool FWD_FETCH_AHEAD = false;
  static constexpr bool XCD_GROUP = false;  // (never measured for these kernels: placement only, but it moves their time)
  typedef unsigned char Lds;
  typedef unsigned char* RowTile;  // (one image serves the row reads and the transposing reads)
  typedef unsigned char* ColTile;

  // staging: thread -> rows r, r + 32 (r = tid >> 3), the 16-byte chunk c = tid & 7
  static __device__ __forceinline__ int stage_col() { return (threadIdx.x & 7) * 8; }
  static __device__ __forceinline__ int operand_col(int g) { return 8 * g; }
  struct Stage {
    bf16x8 v[2];
  };
  // (rows beyond T re-read row T - 1: finite values, probability exactly 0 through the mask tile)
  static __device__ __forceinline__ void fetch_kv(Stage& s, const KvSrcT<__bf16>& src, int P, int T, int ld_txt, int t0) {
    const int r = threadIdx.x >> 3;
#pragma unroll
    for (int i = 0; i < 2; ++i) s.v[i] = *reinterpret_cast<const bf16x8*>(kv_row_ptr(src, min(t0 + r + 32 * i, T - 1), P, ld_txt));
  }
  // rows q0 + r (clamped to n - 1) of Q (row stride 3 H), dO and O (row stride H)
  static __device__ __forceinline__ void fetch_rows(Stage& q, Stage& d, Stage& o, const __bf16* qsrc, const __bf16* dsrc, const __bf16* osrc,
                                                    int H, int q0, int n) {
    const int r = threadIdx.x >> 3;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int qq = min(q0 + r + 32 * i, n - 1);
      q.v[i] = *reinterpret_cast<const bf16x8*>(qsrc + (long)qq * 3 * H);
      d.v[i] = *reinterpret_cast<const bf16x8*>(dsrc + (long)qq * H);
      o.v[i] = *reinterpret_cast<const bf16x8*>(osrc + (long)qq * H);
    }
  }
  static __device__ __forceinline__ void store(unsigned char* tile, const Stage& s) {
    const int c = threadIdx.x & 7, r = threadIdx.x >> 3;
#pragma unroll
    for (int i = 0; i < 2; ++i) *reinterpret_cast<bf16x8*>(tile + tile_off(r + 32 * i, c)) = s.v[i];
  }
  struct StageDelta {
    float s[2];
    __device__ __forceinline__ void reduce(const Stage& o, const Stage& d) {
#pragma unroll
      for (int i = 0; i < 2; ++i) s[i] = dot8(d.v[i], o.v[i]);
#pragma unroll
      for (int i = 0; i < 2; ++i) {  // the 8 threads of a row are 8 consecutive lanes
        s[i] += __shfl_xor(s[i], 1, 64);
        s[i] += __shfl_xor(s[i], 2, 64);
        s[i] += __shfl_xor(s[i], 4, 64);
      }
    }
    __device__ __forceinline__ void store(float* del_s) const {
      if ((threadIdx.x & 7) == 0) {
        del_s[threadIdx.x >> 3] = s[0];
        del_s[(threadIdx.x >> 3) + 32] = s[1];
      }
    }
  };

  struct Operand {
    bf16x8 k[2];
  };
  static __device__ __forceinline__ Operand load_operand(const __bf16* p) {
    Operand x;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) x.k[ks] = *reinterpret_cast<const bf16x8*>(p + 32 * ks);
    return x;
  }
  static __device__ __forceinline__ Operand load_operand_dot(const __bf16* p, const __bf16* op, float& dot) {
    Operand x;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      x.k[ks] = *reinterpret_cast<const bf16x8*>(p + 32 * ks);
      dot += dot8(x.k[ks], *reinterpret_cast<const bf16x8*>(op + 32 * ks));
    }
    return x;
  }

  static __device__ __forceinline__ f32x4 rows_dot(const unsigned char* tile, int blk, const Operand& x, int lr, int g) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) acc = MFMA_BF(row_frag(tile, blk, ks, lr, g), x.k[ks], acc);
    return acc;
  }
  static __device__ __forceinline__ void rows_dot2(const unsigned char* tile0, const Operand& x0, f32x4& r0, const unsigned char* tile1,
                                                   const Operand& x1, f32x4& r1, int blk, int lr, int g) {
    r0 = r1 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      r0 = MFMA_BF(row_frag(tile0, blk, ks, lr, g), x0.k[ks], r0);
      r1 = MFMA_BF(row_frag(tile1, blk, ks, lr, g), x1.k[ks], r1);
    }
  }
  // The whole tile's probabilities first, then two 16-row blocks per product: slot u = the register pair p[2u], p[2u + 1] rounded to
  // bf16, k-depth 32.
  static constexpr int FOLD = 4;
  static __device__ __forceinline__ void cols_acc(const unsigned char* tile, int, const f32x4* p, int nsub, int lane, f32x4 (&acc)[4]) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (2 * u < nsub) {
        const bf16x8 b = pack8(p[2 * u], p[2 * u + 1]);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) acc[dt] = MFMA_BF(tr_frag(tile, u, dt, lane), b, acc[dt]);
      }
    }
  }
  static __device__ __forceinline__ void cols_acc2(const unsigned char* tile0, const f32x4* p0, f32x4 (&acc0)[4], const unsigned char* tile1,
                                                   const f32x4* p1, f32x4 (&acc1)[4], int, int nsub, int lane) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (2 * u < nsub) {
        const bf16x8 b0 = pack8(p0[2 * u], p0[2 * u + 1]), b1 = pack8(p1[2 * u], p1[2 * u + 1]);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          acc0[dt] = MFMA_BF(tr_frag(tile0, u, dt, lane), b0, acc0[dt]);
          acc1[dt] = MFMA_BF(tr_frag(tile1, u, dt, lane), b1, acc1[dt]);
        }
      }
    }
  }

  // Output hooks.  No delta leaves the dQ side and it has neither of the fp32 kernels' whole-tile exits; instead every block writes
  // the column sums of its rows -- zeros from a block that leaves before its loop.
  static __device__ __forceinline__ bool tile_without_gradient(const Operand&, bool, float*) { return false; }
  static __device__ __forceinline__ bool dq_tail_exit(const Args&) { return false; }
  static __device__ __forceinline__ void store_delta(const Args&, long, float) {}
  // x [4] (the MFMA result layout: d = 16 dt + 4 g + r of this lane's row) summed over the 16 rows of a wave -> red [wave][64]
  static __device__ __forceinline__ void wave_col_sums(const f32x4 (&x)[4], bool ok, float* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = ok ? x[dt][r] : 0.f;
        v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64); v += __shfl_xor(v, 8, 64);
        if ((lane & 15) == 0) red[wave * 64 + 16 * dt + 4 * (lane >> 4) + r] = v;
      }
  }
  // (the sentence index as a scalar: as a 64-bit lane value it would hold a register pair through the whole tile loop, and the
  // backward kernel sits at 168 VGPRs, the last count that leaves three waves per SIMD)
  static __device__ __forceinline__ float* partq_row(const Args& a, int qtile, int b, int h) {
    return a.partq + ((long)__builtin_amdgcn_readfirstlane(b) * ((a.S + 63) / 64) + qtile) * a.H + h * D;
  }
  // (rows of partkv per sentence: the padded key count, whatever the layout)
  static __device__ __forceinline__ float* partkv_row(const Args& a, int ktile, int b, int h) {
    return a.partkv + ((long)__builtin_amdgcn_readfirstlane(b) * ((a.P + a.S + 63) / 64) + ktile) * 2 * a.H + h * D;
  }
  static __device__ __forceinline__ void dq_sums_zero(const Args& a, int qtile, int b, int h) {
    if (threadIdx.x < 64) partq_row(a, qtile, b, h)[threadIdx.x] = 0.f;
  }
  // column sums of this block's dQ rows (the query-bias gradient): over the 16 query lanes, then the 4 waves
  static __device__ __forceinline__ void dq_sums(const Args& a, int qtile, int b, int h, const f32x4 (&dq)[4], bool qok, float* red) {
    __syncthreads();
    wave_col_sums(dq, qok, red);
    __syncthreads();
    if (threadIdx.x < 64)
      partq_row(a, qtile, b, h)[threadIdx.x] = red[threadIdx.x] + red[64 + threadIdx.x] + red[128 + threadIdx.x] + red[192 + threadIdx.x];
  }
  static __device__ __forceinline__ void dkv_sums_zero(const Args& a, int ktile, int b, int h) {
    if (threadIdx.x < 128) partkv_row(a, ktile, b, h)[(threadIdx.x >> 6) * a.H + (threadIdx.x & 63)] = 0.f;
  }
  // column sums over this block's TEXT keys (the key / value bias gradients): dK through red [0 .. 255], dV through red [256 .. 511]
  static __device__ __forceinline__ void dkv_sums(const Args& a, int ktile, int b, int h, const f32x4 (&dk)[4], const f32x4 (&dv)[4],
                                                  bool is_text, float* red) {
    __syncthreads();
    wave_col_sums(dk, is_text, red);
    wave_col_sums(dv, is_text, red + 256);
    __syncthreads();
    if (threadIdx.x < 128) {
      const int which = threadIdx.x >> 6, d = threadIdx.x & 63;
      const float* rr = red + which * 256 + d;
      partkv_row(a, ktile, b, h)[which * a.H + d] = rr[0] + rr[64] + rr[128] + rr[192];
    }
  }
};

__global__ __launch_bounds__(256) void attn_bf16_fwd_kernel(Args a) {
  __shared__ __attribute__((aligned(16))) unsigned char Ks[KT * 128];
  __shared__ __attribute__((aligned(16))) unsigned char Vs[KT * 128];
  __shared__ __attribute__((aligned(16))) float Ms[KT];
  __shared__ int t_eff_slot;
  attn_fwd_body<Bf16>(a, Ks, Vs, Ms, &t_eff_slot);
}

__global__ __launch_bounds__(256, 2) void attn_bf16_bwd_kernel(Args a, int nq) {
  __shared__ __attribute__((aligned(16))) unsigned char tile0[KT * 128];
  __shared__ __attribute__((aligned(16))) unsigned char tile1[KT * 128];
  __shared__ __attribute__((aligned(16))) float small[3 * KT];
  __shared__ __attribute__((aligned(16))) float red[8 * 64];
  __shared__ int t_eff_slot;
  attn_bwd_body<Bf16>(a, nq, tile0, tile1, small, red, &t_eff_slot);
}

// ... with a per-sentence prefix-slot mask on packed rows (mask_at<PM>; pmask is an argument of its own: the kernels above keep
// their argument block and their code)
__global__ __launch_bounds__(256) void attn_bf16_fwd_pm_kernel(Args a, const float* pmask) {
  __shared__ __attribute__((aligned(16))) unsigned char Ks[KT * 128];
  __shared__ __attribute__((aligned(16))) unsigned char Vs[KT * 128];
  __shared__ __attribute__((aligned(16))) float Ms[KT];
  __shared__ int t_eff_slot;
  attn_fwd_body<Bf16, true>(a, Ks, Vs, Ms, &t_eff_slot, pmask);
}

__global__ __launch_bounds__(256, 2) void attn_bf16_bwd_pm_kernel(Args a, int nq, const float* pmask) {
  __shared__ __attribute__((aligned(16))) unsigned char tile0[KT * 128];
  __shared__ __attribute__((aligned(16))) unsigned char tile1[KT * 128];
  __shared__ __attribute__((aligned(16))) float small[3 * KT];
  __shared__ __attribute__((aligned(16))) float red[8 * 64];
  __shared__ int t_eff_slot;
  attn_bwd_body<Bf16, true>(a, nq, tile0, tile1, small, red, &t_eff_slot, pmask);
}

static int check(const Args& a) {
  const int rc = attn_check(a);
  if (rc) return rc;
  if (((uintptr_t)a.qkv | (uintptr_t)a.pk | (uintptr_t)a.pv) & 15) return MTVAF_ERR_ALIGN;
  return MTVAF_OK;
}

}  // namespace ab
}  // namespace mtvaf

using namespace mtvaf;

extern "C" {

static int attn16_fwd_launch(const void* qkv16, const void* pk16, const void* pv16, const float* addmask, const int* cu, int pad_rows,
                             void* ctx16, float* lse, int B, int S, int P, int NH, int head_dim, float p_drop, uint64_t seed, uint64_t offset,
                             hipStream_t st, const float* pmask = nullptr) {
  if (head_dim != D) return MTVAF_ERR_SHAPE;
  ab::Args a{};
  a.qkv = static_cast<const __bf16*>(qkv16); a.pk = static_cast<const __bf16*>(pk16); a.pv = static_cast<const __bf16*>(pv16);
  a.addmask = addmask; a.cu = cu; a.pad_rows = pad_rows; a.ctx = static_cast<__bf16*>(ctx16); a.lse = lse;
  attn_fill_common(a, B, S, P, NH, p_drop, seed, offset);
  int rc = ab::check(a);
  if (rc) return rc;
  if (!ctx16 || !lse || (!addmask && !cu) || pad_rows < 0 || (pad_rows && !cu)) return MTVAF_ERR_ARG;
  const dim3 grid((S + 63) / 64, NH, B + (pad_rows > 0 ? 1 : 0));
  if (pmask) hipLaunchKernelGGL(ab::attn_bf16_fwd_pm_kernel, grid, dim3(256), 0, st, a, pmask);
  else hipLaunchKernelGGL(ab::attn_bf16_fwd_kernel, grid, dim3(256), 0, st, a);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

static int attn16_bwd_launch(const void* dctx16, const void* qkv16, const void* pk16, const void* pv16, const float* addmask,
                             const int* cu, int pad_rows, const void* ctx16, const float* lse, void* dqkv16, float* dpk, float* dpv, float* partq,
                             float* partkv, int B, int S, int P, int NH, int head_dim, float p_drop, uint64_t seed, uint64_t offset,
                             hipStream_t st, int zero_tail = 0, const float* pmask = nullptr) {
  if (head_dim != D) return MTVAF_ERR_SHAPE;
  ab::Args a{};
  a.zero_tail = zero_tail;
  a.qkv = static_cast<const __bf16*>(qkv16); a.pk = static_cast<const __bf16*>(pk16); a.pv = static_cast<const __bf16*>(pv16);
  a.addmask = addmask; a.cu = cu; a.pad_rows = pad_rows; a.ctx = static_cast<__bf16*>(const_cast<void*>(ctx16)); a.lse = const_cast<float*>(lse);
  a.dctx = static_cast<const __bf16*>(dctx16); a.dqkv = static_cast<__bf16*>(dqkv16); a.dpk = dpk; a.dpv = dpv;
  a.partq = partq; a.partkv = partkv;
  attn_fill_common(a, B, S, P, NH, p_drop, seed, offset);
  int rc = ab::check(a);
  if (rc) return rc;
  if (!dctx16 || !ctx16 || !lse || !dqkv16 || !partq || !partkv || (!addmask && !cu)) return MTVAF_ERR_ARG;
  if (P > 0 && (!dpk || !dpv)) return MTVAF_ERR_ARG;
  if (((uintptr_t)dctx16 | (uintptr_t)ctx16 | (uintptr_t)dqkv16) & 15) return MTVAF_ERR_ALIGN;
  if (pad_rows < 0 || (pad_rows && !cu)) return MTVAF_ERR_ARG;
  const int nq = (S + 63) / 64;
  const dim3 grid(nq + (P + S + 63) / 64, NH, B + (pad_rows > 0 ? 1 : 0));
  if (pmask) hipLaunchKernelGGL(ab::attn_bf16_bwd_pm_kernel, grid, dim3(256), 0, st, a, nq, pmask);
  else hipLaunchKernelGGL(ab::attn_bf16_bwd_kernel, grid, dim3(256), 0, st, a, nq);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

// ctx16 [B*S,H] bf16, lse [B,NH,S] <- attention over [prefix ; text] keys; qkv16 [B*S,3H] / pk16, pv16 [B,P*H] bf16.
int mtvaf_prefix_attn_bf16_fwd(const void* qkv16, const void* pk16, const void* pv16, const float* addmask, void* ctx16,
                               float* lse, int B, int S, int P, int NH, int head_dim, float p_drop, uint64_t seed,
                               uint64_t offset, hipStream_t st) {
  if (!addmask) return MTVAF_ERR_ARG;
  return attn16_fwd_launch(qkv16, pk16, pv16, addmask, nullptr, 0, ctx16, lse, B, S, P, NH, head_dim, p_drop, seed, offset, st);
}

// dqkv16 [B*S,3H] bf16 (all three column blocks overwritten), dpk / dpv [B,P*H] fp32 <- gradients.
// partq [B*ceil(S/64), H] and partkv [B*ceil((P+S)/64), 2H] fp32: per-block column sums of dQ and of dK | dV (text keys):
// summed over their rows they are the Q / K / V bias gradients.
int mtvaf_prefix_attn_bf16_bwd(const void* dctx16, const void* qkv16, const void* pk16, const void* pv16,
                               const float* addmask, const void* ctx16, const float* lse, void* dqkv16, float* dpk,
                               float* dpv, float* partq, float* partkv, int B, int S, int P, int NH, int head_dim,
                               float p_drop, uint64_t seed, uint64_t offset, hipStream_t st) {
  if (!addmask) return MTVAF_ERR_ARG;
  return attn16_bwd_launch(dctx16, qkv16, pk16, pv16, addmask, nullptr, 0, ctx16, lse, dqkv16, dpk, dpv, partq, partkv, B, S, P, NH,
                           head_dim, p_drop, seed, offset, st);
}

// mtvaf_prefix_attn_bf16_bwd for callers that vouch (zero_tail != 0) that dctx is exactly zero behind each sentence's last
// unmasked position (see mtvaf_prefix_attn_bwd_tail): same bits, the key side's query loop stops there.
int mtvaf_prefix_attn_bf16_bwd_tail(const void* dctx16, const void* qkv16, const void* pk16, const void* pv16, const float* addmask,
                                    const void* ctx16, const float* lse, void* dqkv16, float* dpk, float* dpv, float* partq,
                                    float* partkv, int B, int S, int P, int NH, int head_dim, float p_drop, uint64_t seed,
                                    uint64_t offset, int zero_tail, hipStream_t st) {
  if (!addmask) return MTVAF_ERR_ARG;
  return attn16_bwd_launch(dctx16, qkv16, pk16, pv16, addmask, nullptr, 0, ctx16, lse, dqkv16, dpk, dpv, partq, partkv, B, S, P, NH,
                           head_dim, p_drop, seed, offset, st, zero_tail);
}

// PACKED token rows (padding-free execution; see mtvaf_prefix_attn_varlen_fwd): cu [B+1] int32 row offsets, no mask read;
// partq / partkv keep their padded row counts (blocks beyond a sentence write zeros).
int mtvaf_prefix_attn_bf16_varlen_fwd(const void* qkv16, const void* pk16, const void* pv16, const int* cu, int pad_rows, void* ctx16,
                                      float* lse, int B, int S, int P, int NH, int head_dim, float p_drop, uint64_t seed,
                                      uint64_t offset, hipStream_t st) {
  if (!cu) return MTVAF_ERR_ARG;
  return attn16_fwd_launch(qkv16, pk16, pv16, nullptr, cu, pad_rows, ctx16, lse, B, S, P, NH, head_dim, p_drop, seed, offset, st);
}

int mtvaf_prefix_attn_bf16_varlen_bwd(const void* dctx16, const void* qkv16, const void* pk16, const void* pv16, const int* cu,
                                      int pad_rows, const void* ctx16, const float* lse, void* dqkv16, float* dpk, float* dpv, float* partq,
                                      float* partkv, int B, int S, int P, int NH, int head_dim, float p_drop, uint64_t seed,
                                      uint64_t offset, hipStream_t st) {
  if (!cu) return MTVAF_ERR_ARG;
  return attn16_bwd_launch(dctx16, qkv16, pk16, pv16, nullptr, cu, pad_rows, ctx16, lse, dqkv16, dpk, dpv, partq, partkv, B, S, P, NH,
                           head_dim, p_drop, seed, offset, st);
}

// ... with a per-sentence prefix-slot mask (see mtvaf_prefix_attn_varlen_fwd_pm): pmask [B, P] fp32 additive, pmask_len = B * P;
// pmask == NULL: the launch of mtvaf_prefix_attn_bf16_varlen_fwd / _bwd.
int mtvaf_prefix_attn_bf16_varlen_fwd_pm(const void* qkv16, const void* pk16, const void* pv16, const int* cu, int pad_rows,
                                         const float* pmask, long pmask_len, void* ctx16, float* lse, int B, int S, int P, int NH,
                                         int head_dim, float p_drop, uint64_t seed, uint64_t offset, hipStream_t st) {
  if (!cu) return MTVAF_ERR_ARG;
  if (pmask && (P <= 0 || B <= 0 || pmask_len != (long)B * P)) return MTVAF_ERR_ARG;
  return attn16_fwd_launch(qkv16, pk16, pv16, nullptr, cu, pad_rows, ctx16, lse, B, S, P, NH, head_dim, p_drop, seed, offset, st, pmask);
}

int mtvaf_prefix_attn_bf16_varlen_bwd_pm(const void* dctx16, const void* qkv16, const void* pk16, const void* pv16, const int* cu,
                                         int pad_rows, const float* pmask, long pmask_len, const void* ctx16, const float* lse,
                                         void* dqkv16, float* dpk, float* dpv, float* partq, float* partkv, int B, int S, int P, int NH,
                                         int head_dim, float p_drop, uint64_t seed, uint64_t offset, hipStream_t st) {
  if (!cu) return MTVAF_ERR_ARG;
  if (pmask && (P <= 0 || B <= 0 || pmask_len != (long)B * P)) return MTVAF_ERR_ARG;
  return attn16_bwd_launch(dctx16, qkv16, pk16, pv16, nullptr, cu, pad_rows, ctx16, lse, dqkv16, dpk, dpv, partq, partkv, B, S, P, NH,
                           head_dim, p_drop, seed, offset, st, 0, pmask);
}

}  // extern "C"
