// fp32 prefix self-attention with its four (forward) / ten (backward) matrix products formed as SPLIT bf16 products -- the fp32
// arithmetic of csrc/gemm_f32x3.hip / gemm_f32p.hip (every fp32 operand value x = x1 + x2 + x3, three RNE bf16 planes; a product
// a.b = a3 b1 + a1 b3 + a2 b2 + a2 b1 + a1 b2 + a1 b1 on v_mfma_f32_16x16x32_bf16, fp32 accumulation, smallest terms first; the
// dropped terms are below 2^-26 |a||b|) -- instead of v_mfma_f32_16x16x4_f32, which runs at 1/16 of the bf16 rate:
//   softmax(Q.[Kp;K]^T / sqrt(D) + mask) . [Vp;V]     models/modeling_bert.py:282-286, 303, 320-337
// Round 6.  Why: on the CUs that hold a launch's long sentences the fp32 matrix pipe is the critical path of the fp32-pipe kernels
// (timing-only ablation builds of that round, since removed; profiles/r06_attention_ablation.txt: 44 % of the forward launch is its QK^T and PV
// products); six bf16 products per fp32 product need 2.7 x fewer matrix cycles.
//
// Same interface (AttnArgs), launch geometry, key order, masking, log2-domain softmax, dropout hash, outputs (fp32 + optional plane
// images) and contracts as attention.hip; the structure is that of attention_bf16.hip (scores TRANSPOSED, S^T[key][q] = K.Q^T: a
// query lives on a lane; the C layout of the score block IS the B operand of O^T[d][q] = V^T.P^T under the k-slot definition
// (g, j) -> key 16 (2u + (j >> 2)) + 4g + (j & 3); V^T by transposing LDS reads) with every operand as three planes:
//   * K / V (Q / dO on the key side of the backward pass) tiles: fp32 rows from global memory, split while they are staged -- three
//     [64][64] bf16 images per tile (the image of attention_bf16.hip: 16-byte chunk c of row r at c ^ (((r >> 1) & 3) << 1));
//   * Q / dO (K / V on the key side) fragments: 8 consecutive d per lane, split once per block into registers;
//   * probabilities, dS: split in registers (their fp32 values are the MFMA result layout already).
//
// The kernel bodies are those of csrc/attention_skeleton.h; this file provides their split-product arithmetic.
#include "attention_skeleton.h"

namespace mtvaf {
namespace as3 {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

#define MFMA_BF(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16((a), (b), (c), 0, 0, 0)

constexpr int PLANE_B = KT * 128;  // one [64][64] bf16 plane image: 8 KiB
constexpr int TILE_B = 3 * PLANE_B;

struct P3 {  // the three planes of 8 fp32 values
  bf16x8 p[3];
};

// 8 fp32 values -> their three bf16 planes (RNE at each level: the split of csrc/planes.h, bit for bit)
__device__ __forceinline__ P3 split8(f32x4 a, f32x4 b) {
  // (as ROUNDED fp32 values: under -ffp-contract=fast a residual must not fuse with the arithmetic that produced its operand)
  asm volatile("" : "+v"(a.x), "+v"(a.y), "+v"(a.z), "+v"(a.w), "+v"(b.x), "+v"(b.y), "+v"(b.z), "+v"(b.w));
  unsigned h[4], m[4], l[4];
  pl_split(pl_f32x2{a.x, a.y}, h[0], m[0], l[0]);
  pl_split(pl_f32x2{a.z, a.w}, h[1], m[1], l[1]);
  pl_split(pl_f32x2{b.x, b.y}, h[2], m[2], l[2]);
  pl_split(pl_f32x2{b.z, b.w}, h[3], m[3], l[3]);
  P3 r;
  r.p[0] = __builtin_bit_cast(bf16x8, uint4{h[0], h[1], h[2], h[3]});
  r.p[1] = __builtin_bit_cast(bf16x8, uint4{m[0], m[1], m[2], m[3]});
  r.p[2] = __builtin_bit_cast(bf16x8, uint4{l[0], l[1], l[2], l[3]});
  return r;
}

// A operand of a "rows x d" product: row 16 blk + (lane & 15), the 8 d values 32 ks + 8 g .. + 7 of plane pl
__device__ __forceinline__ bf16x8 row_frag(const unsigned char* tile, int pl, int blk, int ks, int lr, int g) {
  return *reinterpret_cast<const bf16x8*>(tile + pl * PLANE_B + tile_off(16 * blk + lr, 4 * ks + g));
}
// A operand of a "d x rows" product (transposing read): d = 16 dt + (lane & 15), k-slot (g, j) = tile row 16 (2u + (j >> 2)) + 4g + (j & 3)
__device__ __forceinline__ bf16x8 tr_frag(const unsigned char* tile, int pl, int u, int dt, int lane) {
  const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
  const int r0 = 32 * u + 4 * g + q, r1 = r0 + 16;
  const int c = 2 * dt + (p >> 1), e = 8 * (p & 1);
  const unsigned char* t = tile + pl * PLANE_B;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(t + tile_off(r0, c) + e));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(t + tile_off(r1, c) + e));
  return __builtin_bit_cast(bf16x8, (s16x8)__builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// the six plane pairs of a split product (A plane, B plane), smallest terms first: a3 b1, a1 b3, a2 b2, a2 b1, a1 b2, a1 b1
#define AS3_PAIRS constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0}

// The split-product arithmetic: a tile is three [64][64] bf16 plane images, split while it is staged; the operand of a row is its
// 64 values as planes, 8 consecutive d per lane at 32 ks + 8 g .. + 7 (ks = 0, 1); every product is six bf16 MFMA products.
struct Split3 : F32Io {
  typedef unsigned char Lds;
  typedef unsigned char* RowTile;  // (one image serves the row reads and the transposing reads)
  typedef unsigned char* ColTile;

  // staging: thread -> rows r, r + 32 (r = tid >> 3), the 8 values of chunk c = tid & 7
  static __device__ __forceinline__ int stage_col() { return (threadIdx.x & 7) * 8; }
  static __device__ __forceinline__ int operand_col(int g) { return 8 * g; }
  struct Stage {
    f32x4 v[2][2];
  };
  // (rows beyond T re-read row T - 1: finite values, probability exactly 0 through the mask tile)
  static __device__ __forceinline__ void fetch_kv(Stage& s, const KvSrc& src, int P, int T, int ld_txt, int t0) {
    const int r = threadIdx.x >> 3;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const float* row = kv_row_ptr(src, min(t0 + r + 32 * i, T - 1), P, ld_txt);
      s.v[i][0] = *reinterpret_cast<const f32x4*>(row);
      s.v[i][1] = *reinterpret_cast<const f32x4*>(row + 4);
    }
  }
  // rows q0 + r (clamped to n - 1) of Q (row stride 3 H), dO and O (row stride H)
  static __device__ __forceinline__ void fetch_rows(Stage& q, Stage& d, Stage& o, const float* qsrc, const float* dsrc, const float* osrc, int H,
                                                    int q0, int n) {
    const int r = threadIdx.x >> 3;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int qq = min(q0 + r + 32 * i, n - 1);
      q.v[i][0] = *reinterpret_cast<const f32x4*>(qsrc + (long)qq * 3 * H);
      q.v[i][1] = *reinterpret_cast<const f32x4*>(qsrc + (long)qq * 3 * H + 4);
      d.v[i][0] = *reinterpret_cast<const f32x4*>(dsrc + (long)qq * H);
      d.v[i][1] = *reinterpret_cast<const f32x4*>(dsrc + (long)qq * H + 4);
      o.v[i][0] = *reinterpret_cast<const f32x4*>(osrc + (long)qq * H);
      o.v[i][1] = *reinterpret_cast<const f32x4*>(osrc + (long)qq * H + 4);
    }
  }
  static __device__ __forceinline__ void store(unsigned char* tile, const Stage& s) {
    const int c = threadIdx.x & 7, r = threadIdx.x >> 3;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const P3 q = split8(s.v[i][0], s.v[i][1]);
      const int o = tile_off(r + 32 * i, c);
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) *reinterpret_cast<bf16x8*>(tile + pl * PLANE_B + o) = q.p[pl];
    }
  }
  struct StageDelta {
    float s[2];
    __device__ __forceinline__ void reduce(const Stage& o, const Stage& d) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const f32x4 x0 = o.v[i][0] * d.v[i][0], x1 = o.v[i][1] * d.v[i][1];
        s[i] = (x0.x + x0.y + x0.z + x0.w) + (x1.x + x1.y + x1.z + x1.w);
      }
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
    P3 k[2];
  };
  static __device__ __forceinline__ Operand load_operand(const float* p) {
    Operand x;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
      x.k[ks] = split8(*reinterpret_cast<const f32x4*>(p + 32 * ks), *reinterpret_cast<const f32x4*>(p + 32 * ks + 4));
    return x;
  }
  static __device__ __forceinline__ Operand load_operand_dot(const float* p, const float* op, float& dot) {
    Operand x;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const f32x4 d0 = *reinterpret_cast<const f32x4*>(p + 32 * ks), d1 = *reinterpret_cast<const f32x4*>(p + 32 * ks + 4);
      const f32x4 o0 = *reinterpret_cast<const f32x4*>(op + 32 * ks), o1 = *reinterpret_cast<const f32x4*>(op + 32 * ks + 4);
      dot += o0.x * d0.x + o0.y * d0.y + o0.z * d0.z + o0.w * d0.w + o1.x * d1.x + o1.y * d1.y + o1.z * d1.z + o1.w * d1.w;
      x.k[ks] = split8(d0, d1);
    }
    return x;
  }

  static __device__ __forceinline__ f32x4 rows_dot(const unsigned char* tile, int blk, const Operand& b, int lr, int g) {
    bf16x8 a[3][2];
#pragma unroll
    for (int pl = 0; pl < 3; ++pl)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) a[pl][ks] = row_frag(tile, pl, blk, ks, lr, g);
    AS3_PAIRS;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 6; ++t)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) acc = MFMA_BF(a[PA[t]][ks], b.k[ks].p[PB[t]], acc);
    return acc;
  }
  static __device__ __forceinline__ void rows_dot2(const unsigned char* tile0, const Operand& x0, f32x4& r0, const unsigned char* tile1,
                                                   const Operand& x1, f32x4& r1, int blk, int lr, int g) {
    r0 = rows_dot(tile0, blk, x0, lr, g);
    r1 = rows_dot(tile1, blk, x1, lr, g);
  }
  // The whole tile's probabilities first, then two 16-row blocks per product: slot u = the split of the register pair p[2u], p[2u + 1],
  // k-depth 32.
  static constexpr int FOLD = 4;
  static __device__ __forceinline__ void cols_slot(const unsigned char* tile, int u, const f32x4* p, int lane, f32x4 (&acc)[4]) {
    const P3 b = split8(p[2 * u], p[2 * u + 1]);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      bf16x8 a[3];
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) a[pl] = tr_frag(tile, pl, u, dt, lane);
      AS3_PAIRS;
#pragma unroll
      for (int t = 0; t < 6; ++t) acc[dt] = MFMA_BF(a[PA[t]], b.p[PB[t]], acc[dt]);
    }
  }
  static __device__ __forceinline__ void cols_acc(const unsigned char* tile, int, const f32x4* p, int nsub, int lane, f32x4 (&acc)[4]) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (2 * u < nsub) cols_slot(tile, u, p, lane, acc);
    }
  }
  static __device__ __forceinline__ void cols_acc2(const unsigned char* tile0, const f32x4* p0, f32x4 (&acc0)[4], const unsigned char* tile1,
                                                   const f32x4* p1, f32x4 (&acc1)[4], int, int nsub, int lane) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (2 * u < nsub) {
        cols_slot(tile0, u, p0, lane, acc0);
        cols_slot(tile1, u, p1, lane, acc1);
      }
    }
  }

  // (the dQ loop is at its register limit: no test for an all-zero dO tile here, see the fp32-pipe arithmetic)
  static __device__ __forceinline__ bool tile_without_gradient(const Operand&, bool, float*) { return false; }
};

__global__ __launch_bounds__(256) void attn_f32s_fwd_kernel(AttnArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char Ks[TILE_B];
  __shared__ __attribute__((aligned(16))) unsigned char Vs[TILE_B];
  __shared__ __attribute__((aligned(16))) float Ms[KT];
  __shared__ int t_eff_slot;
  attn_fwd_body<Split3>(a, Ks, Vs, Ms, &t_eff_slot);
}

__global__ __launch_bounds__(256) void attn_f32s_probs_kernel(AttnArgs a, ProbsOut o) {
  __shared__ __attribute__((aligned(16))) unsigned char Ks[TILE_B];
  __shared__ __attribute__((aligned(16))) float Ps[KT * LDP];
  __shared__ __attribute__((aligned(16))) float Ms[KT];
  __shared__ int t_eff_slot;
  attn_probs_body<Split3>(a, o, Ks, Ps, Ms, &t_eff_slot);
}

__global__ __launch_bounds__(256, 2) void attn_f32s_bwd_kernel(AttnArgs a, int nq) {
  __shared__ __attribute__((aligned(16))) unsigned char tile0[TILE_B];
  __shared__ __attribute__((aligned(16))) unsigned char tile1[TILE_B];
  __shared__ __attribute__((aligned(16))) float small[3 * KT];
  __shared__ int t_eff_slot;
  attn_bwd_body<Split3>(a, nq, tile0, tile1, small, nullptr, &t_eff_slot);
}

// ... with a per-sentence prefix-slot mask on packed rows (mask_at<PM>; pmask is an argument of its own: the kernels above keep
// their argument block and their code)
__global__ __launch_bounds__(256) void attn_f32s_fwd_pm_kernel(AttnArgs a, const float* pmask) {
  __shared__ __attribute__((aligned(16))) unsigned char Ks[TILE_B];
  __shared__ __attribute__((aligned(16))) unsigned char Vs[TILE_B];
  __shared__ __attribute__((aligned(16))) float Ms[KT];
  __shared__ int t_eff_slot;
  attn_fwd_body<Split3, true>(a, Ks, Vs, Ms, &t_eff_slot, pmask);
}

__global__ __launch_bounds__(256, 2) void attn_f32s_bwd_pm_kernel(AttnArgs a, int nq, const float* pmask) {
  __shared__ __attribute__((aligned(16))) unsigned char tile0[TILE_B];
  __shared__ __attribute__((aligned(16))) unsigned char tile1[TILE_B];
  __shared__ __attribute__((aligned(16))) float small[3 * KT];
  __shared__ int t_eff_slot;
  attn_bwd_body<Split3, true>(a, nq, tile0, tile1, small, nullptr, &t_eff_slot, pmask);
}

}  // namespace as3

int launch_attn_f32s_fwd(const AttnArgs& a, dim3 grid, hipStream_t st, const float* pmask) {
  if (pmask) hipLaunchKernelGGL(as3::attn_f32s_fwd_pm_kernel, grid, dim3(256), 0, st, a, pmask);
  else hipLaunchKernelGGL(as3::attn_f32s_fwd_kernel, grid, dim3(256), 0, st, a);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}
int launch_attn_f32s_probs(const AttnArgs& a, const ProbsOut& o, dim3 grid, hipStream_t st) {
  hipLaunchKernelGGL(as3::attn_f32s_probs_kernel, grid, dim3(256), 0, st, a, o);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}
int launch_attn_f32s_bwd(const AttnArgs& a, int nq, dim3 grid, hipStream_t st, const float* pmask) {
  if (pmask) hipLaunchKernelGGL(as3::attn_f32s_bwd_pm_kernel, grid, dim3(256), 0, st, a, nq, pmask);
  else hipLaunchKernelGGL(as3::attn_f32s_bwd_kernel, grid, dim3(256), 0, st, a, nq);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

}  // namespace mtvaf
