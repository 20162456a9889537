// AdamW update (reference modules/train.py:894-926 builds torch.optim.AdamW groups and
// :621-625 steps them) and the bf16 gradient wire format of mtvaf_amd/parallel.py.  All kernels are HBM-bound
// streams: 16 bytes per lane per access, grid sized to a few waves per SIMD.
//
//   AdamW, per element (decoupled weight decay, bias-corrected, as torch.optim.AdamW):
//     p  -= lr * wd * p
//     m   = m + (1 - b1) * (g - m)            (1 - b rounded once from double, like torch's python scalars)
//     v   = b2 * v + (1 - b2) * g * g
//     p  -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
//   7 fp32 streams per parameter (read p, g, m, v; write p, m, v) = 28 B; an optional bf16 copy of the new
//   parameter (the GEMM operand shadow of the bf16 compute mode) adds 2 B.
//
//   ONE arithmetic: adamw1 states every rounding of the update (explicit fmaf, contraction off inside it), ema1 the one of the
//   average.  Every kernel below reaches them through one float4 step (adamw_step4: 16-byte accesses, non-temporal) or one scalar
//   step (adamw_step1: tails and views off the 16-byte boundary), so an element gets the same bits from every form, on either step,
//   with any combination of the flags.
//
//   FIVE forms, one kernel template each:
//     flat        one buffer                                                         mtvaf_adamw*, mtvaf_adamw_sched
//     planes      one buffer (n % 4 == 0) + the plane images of up to 4 matrices in it   mtvaf_adamw_planes*
//     multi       up to 48 tensors of one parameter group per launch                    mtvaf_adamw_multi*
//     seg         flat with lr and weight decay per segment of the buffer               mtvaf_adamw_seg*
//     planes_seg  planes with lr and weight decay per segment                           mtvaf_adamw_planes_seg*
//   and THREE compile-time flags on each of them:
//     EMA    also keep an exponential moving average of the parameters, on the element just updated:
//            e = fmaf(ema_omd, p_new - e, e),  ema_omd = 1 - decay  -- one more load and one more store, 8 B per parameter, instead
//            of an averaging pass of 12 B after the step.  The average feeds nothing: the shadow and the images are written from p.
//     DEV    read a device clip state {norm, coef, finite, -} (written by mtvaf_grad_clip_finalize, csrc/gradnorm.hip): the gradient
//            is scaled by grad_scale * coef, and with finite == 0 the kernel returns before its first load -- p, m, v, the average,
//            the shadow and the plane images keep their bits.
//     SCHED  read the step's own hyper-parameters from the device: a 32-byte block {lr_factor (double), bc1, bc2_sqrt, ema_omd,
//            overrun, step} that mtvaf_adamw_sched_advance copies out of a host-built table, one row per optimizer step.  The
//            learning rate is (float)(base_lr * lr_factor) -- base_lr travels as a double, so this is the product and the one
//            rounding a LambdaLR followed by the C ABI's float argument performs on the host -- and nothing per-step is left in the
//            kernel arguments: the launches can be captured into a graph and replayed.  A set overrun word (the counter has passed
//            the table) makes a launch write nothing, like a non-finite clip state.
//   The flags only decide where a launch's numbers come from (step_begin) and whether the average is kept; they never reach adamw1.
#include <climits>
#include <type_traits>

#include "common.h"
#include "planes.h"

namespace mtvaf {

struct AdamHyper {
  float lr, beta1, beta2, eps, wd, bc1, bc2_sqrt, grad_scale;
  float omb1, omb2;  // 1 - beta, rounded ONCE from double (as torch does: float(1 - 0.999) != 1.f - float(0.999) by 1.3e-5)
};
static inline AdamHyper make_hyper(float lr, double beta1, double beta2, float eps, float wd, float bc1, float bc2_sqrt,
                                   float grad_scale) {
  return AdamHyper{lr, (float)beta1, (float)beta2, eps, wd, bc1, bc2_sqrt, grad_scale, (float)(1.0 - beta1), (float)(1.0 - beta2)};
}

// The update of one element.  Each line is ONE rounding (sqrtf and / are correctly rounded), so the bits follow from this text and
// not from what the compiler chooses to fuse around it: no product feeds a sum outside an fmaf, and contraction is off in here.
__device__ __forceinline__ void adamw1(float& p, float g, float& m, float& v, const AdamHyper& h) {
#pragma clang fp contract(off)
  const float s = h.grad_scale;              // (DEV: grad_scale * clip coefficient, rounded once in step_begin)
  const float gs = g * s;
  const float d = fmaf(g, s, -m);            // g * s - m in one rounding, NOT gs - m
  m = fmaf(h.omb1, d, m);
  v = fmaf(h.beta2, v, gs * (h.omb2 * gs));
  const float p1 = fmaf(-(h.lr * h.wd), p, p);
  const float den = sqrtf(v) / h.bc2_sqrt + h.eps;
  p = fmaf(-(h.lr / h.bc1), m / den, p1);
}

// the average of one element behind its update: one fma (the difference rounds once, the product and the sum once)
__device__ __forceinline__ float ema1(float e, float p_new, float omd) { return fmaf(omd, p_new - e, e); }

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ bf16x4 to_bf16x4(f32x4 P) { return bf16x4{(__bf16)P.x, (__bf16)P.y, (__bf16)P.z, (__bf16)P.w}; }

// float4 number i of p, g, m, v (and e), every base on a 16-byte boundary; -> the new parameters
// (non-temporal streams: 28 bytes per parameter pass through once per step -- keeping them out of L2 / Infinity Cache leaves the
// GEMM panels of the backward pass this update runs next to (overlap mode) resident)
template <bool EMA>
__device__ __forceinline__ f32x4 adamw_step4(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                             float* __restrict__ v, float* __restrict__ e, float ema_omd, long i, const AdamHyper& h) {
  f32x4 P = __builtin_nontemporal_load(reinterpret_cast<f32x4*>(p) + i);
  const f32x4 G = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(g) + i);
  f32x4 M = __builtin_nontemporal_load(reinterpret_cast<f32x4*>(m) + i);
  f32x4 V = __builtin_nontemporal_load(reinterpret_cast<f32x4*>(v) + i);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float pj = P[j], mj = M[j], vj = V[j];
    adamw1(pj, G[j], mj, vj, h);
    P[j] = pj; M[j] = mj; V[j] = vj;
  }
  reinterpret_cast<f32x4*>(p)[i] = P;  // (read again by the next forward pass)
  __builtin_nontemporal_store(M, reinterpret_cast<f32x4*>(m) + i);
  __builtin_nontemporal_store(V, reinterpret_cast<f32x4*>(v) + i);
  if constexpr (EMA) {  // (touched once per step, like the moments)
    f32x4 E = __builtin_nontemporal_load(reinterpret_cast<f32x4*>(e) + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) E[j] = ema1(E[j], P[j], ema_omd);
    __builtin_nontemporal_store(E, reinterpret_cast<f32x4*>(e) + i);
  }
  return P;
}

// element i: tails, and views into packed parameter storage that are off the 16-byte boundary
template <bool EMA>
__device__ __forceinline__ void adamw_step1(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                            float* __restrict__ v, float* __restrict__ e, float ema_omd, __bf16* __restrict__ ph,
                                            long i, const AdamHyper& h) {
  float P = p[i], M = m[i], V = v[i];
  adamw1(P, g[i], M, V, h);
  p[i] = P; m[i] = M; v[i] = V;
  if constexpr (EMA) e[i] = ema1(e[i], P, ema_omd);
  if (ph) ph[i] = (__bf16)P;
}

// ---- segments: lr and weight decay per stretch of the flat buffer (the seg and planes_seg forms) -------------------------------
// A fine-tuning recipe that exempts biases and LayerNorm weights from weight decay puts two parameter groups inside every encoder
// layer; the layer's flat buffer is then up to 16 consecutive segments with an lr and a weight decay each.  The table travels by
// value in the kernel arguments (33 dwords: it sits in SGPRs), and every lane picks the segment of the float4 it is about to update
// with a branch-free scan -- 15 compares and 30 selects per 16 elements of a stream that moves 112 bytes for them.  Everything
// else of AdamHyper belongs to the launch.
constexpr int ADAM_MAXSEG = 16;
struct AdamSegTable {
  int end4[ADAM_MAXSEG];  // end of segment k in float4 units for k < n - 1; INT_MAX from the last segment on (it ends with the buffer)
  float lr[ADAM_MAXSEG], wd[ADAM_MAXSEG];
  int n;
};
__device__ __forceinline__ void seg_hyper(const AdamSegTable& t, int i4, AdamHyper& h) {
  float lr = t.lr[0], wd = t.wd[0];
#pragma unroll
  for (int k = 0; k + 1 < ADAM_MAXSEG; ++k) {
    const bool past = i4 >= t.end4[k];
    lr = past ? t.lr[k + 1] : lr;
    wd = past ? t.wd[k + 1] : wd;
  }
  h.lr = lr;
  h.wd = wd;
}
// the SCHED forms: the table carries every segment's BASE lr as a double; the step's table of floats is made from it in the kernel
struct AdamSegTableD {
  int end4[ADAM_MAXSEG];
  double lr[ADAM_MAXSEG];
  float wd[ADAM_MAXSEG];
  int n;
};
__device__ __forceinline__ AdamSegTable seg_table_at(const AdamSegTableD& s, double lr_factor) {
  AdamSegTable t;
#pragma unroll
  for (int k = 0; k < ADAM_MAXSEG; ++k) {
    t.end4[k] = s.end4[k];
    t.lr[k] = (float)(s.lr[k] * lr_factor);
    t.wd[k] = s.wd[k];
  }
  t.n = s.n;
  return t;
}

// ---- plane images: up to four row-major matrices inside a flat buffer (an encoder layer's wqkv / wo / w1 / w2) whose pre-split
// operand form (planes.h) is rewritten by the pass that updates them: a float4 of matrix s, at element e of it, is row e / cols,
// columns e % cols .. + 3 of its image -- 6 more bytes written per weight instead of a split pass that reads the 4 again.
struct AdamSegs {
  long b4[4], e4[4];  // the matrix's float4 range in the flat buffer
  int rows[4], cols[4];
  unsigned char* img[4];
  int n;
};
// float4 number i of the flat buffer, as it has just been stored: -> the image of the matrix it lies in, if it lies in one
__device__ __forceinline__ void mats_store4(const AdamSegs& sg, long i, f32x4 P) {
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    if (s < sg.n && i >= sg.b4[s] && i < sg.e4[s]) {
      const long e = (i - sg.b4[s]) * 4;
      const long row = e / sg.cols[s];
      planes_store4(sg.img[s], sg.rows[s], row, (int)(e - row * sg.cols[s]), P);
    }
  }
}

// ---- the two loops ---------------------------------------------------------------------------------------------------------------
// n elements from lane i0 in steps of `stride`: float4 steps while every base is on a 16-byte boundary (the shadow: 8), scalar steps
// otherwise and for the n % 4 elements of the tail.  SEG: lr and weight decay of each float4 from the table (whose host checks leave
// every base aligned and every inner end a multiple of 4: the tail lies in the last segment).
template <bool EMA, bool SEG>
__device__ __forceinline__ void adamw_span(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                           float* __restrict__ v, float* __restrict__ e, float ema_omd, __bf16* __restrict__ ph,
                                           long n, long i0, long stride, AdamHyper h, const AdamSegTable* t) {
  const bool vec = SEG || (((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)e) & 15) == 0) &&
                           (!ph || ((uintptr_t)ph & 7) == 0));
  const long n4 = vec ? (n >> 2) : 0;
  for (long i = i0; i < n4; i += stride) {
    if constexpr (SEG) seg_hyper(*t, (int)i, h);
    const f32x4 P = adamw_step4<EMA>(p, g, m, v, e, ema_omd, i, h);
    if (ph) reinterpret_cast<bf16x4*>(ph)[i] = to_bf16x4(P);
  }
  if constexpr (SEG) seg_hyper(*t, (int)n4, h);
  for (long i = (n4 << 2) + i0; i < n; i += stride) adamw_step1<EMA>(p, g, m, v, e, ema_omd, ph, i, h);
}

// n4 float4s of a buffer with plane images (every base aligned, no tail: the host checks); the matrices are independent of the
// segments, a matrix may lie across their ends
template <bool EMA, bool SEG>
__device__ __forceinline__ void adamw_planes_span(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                  float* __restrict__ v, float* __restrict__ e, float ema_omd, long n4, AdamHyper h,
                                                  const AdamSegTable* t, const AdamSegs& sg) {
  const long stride = (long)gridDim.x * 256;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    if constexpr (SEG) seg_hyper(*t, (int)i, h);
    mats_store4(sg, i, adamw_step4<EMA>(p, g, m, v, e, ema_omd, i, h));
  }
}

// ---- what a launch knows of the step besides its buffers, and what a kernel does with it before its loop --------------------------
struct SchedRow {      // one optimizer step of the host's table
  double lr_factor;    // what the LambdaLR lambda returns for the step whose lr this update uses
  float bc1, bc2_sqrt, ema_omd;
  int pad;
};
struct SchedCurrent {  // the row of the step being taken, at a fixed address
  double lr_factor;
  float bc1, bc2_sqrt, ema_omd;
  int overrun;         // != 0: the counter is outside 1 .. rows -- every SCHED update returns before its first load
  long step;           // the counter's value, for readers
};
static_assert(sizeof(SchedRow) == 24 && sizeof(SchedCurrent) == 32, "the layout mtvaf_amd/optim.py writes");

// one lane: ++counter, row min(counter, rows) - 1 -> current.  (The row index is clamped on both sides: a counter the caller has
// set below 0 reads row 0 and raises overrun too.)
__global__ void sched_advance_kernel(const SchedRow* __restrict__ table, long rows, long* __restrict__ counter,
                                     SchedCurrent* __restrict__ cur) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const long c = *counter + 1;
  *counter = c;
  long r = (c < rows ? c : rows) - 1;
  if (r < 0) r = 0;
  const SchedRow row = table[r];
  cur->lr_factor = row.lr_factor;
  cur->bc1 = row.bc1;
  cur->bc2_sqrt = row.bc2_sqrt;
  cur->ema_omd = row.ema_omd;
  cur->overrun = (c < 1 || c > rows) ? 1 : 0;
  cur->step = c;
}

struct AdamStep {
  AdamHyper h;
  float ema_omd;            // EMA (SCHED: from cur)
  double base_lr;           // SCHED, unsegmented forms
  const SchedCurrent* cur;  // SCHED
  const float* clip;        // DEV
};
// block-uniform, a few scalar loads.  SCHED: the step's lr, bias corrections and 1 - decay from cur (one IEEE double product, one
// rounding to float: the host's group["lr"] -> c_float).  DEV: the clip coefficient into grad_scale.  false: write nothing
template <bool DEV, bool SCHED>
__device__ __forceinline__ bool step_begin(AdamStep& s) {
  if constexpr (SCHED) {
    if (s.cur->overrun != 0) return false;
    s.h.lr = (float)(s.base_lr * s.cur->lr_factor);
    s.h.bc1 = s.cur->bc1;
    s.h.bc2_sqrt = s.cur->bc2_sqrt;
    s.ema_omd = s.cur->ema_omd;
  }
  if constexpr (DEV) {
    if (s.clip[2] == 0.f) return false;
    s.h.grad_scale *= s.clip[1];
  }
  return true;
}

// ---- the five forms ---------------------------------------------------------------------------------------------------------------
template <bool EMA, bool DEV, bool SCHED>
__global__ __launch_bounds__(256) void adamw_flat_kernel(float* p, const float* g, float* m, float* v, float* e, __bf16* ph, long n,
                                                         AdamStep s) {
  if (!step_begin<DEV, SCHED>(s)) return;
  adamw_span<EMA, false>(p, g, m, v, e, s.ema_omd, ph, n, (long)blockIdx.x * 256 + threadIdx.x, (long)gridDim.x * 256, s.h, nullptr);
}

template <bool EMA, bool DEV, bool SCHED>
__global__ __launch_bounds__(256) void adamw_planes_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, float* __restrict__ e, long n4, AdamStep s,
                                                           AdamSegs sg) {
  if (!step_begin<DEV, SCHED>(s)) return;
  adamw_planes_span<EMA, false>(p, g, m, v, e, s.ema_omd, n4, s.h, nullptr, sg);
}

// several tensors of one parameter group in one launch: blockIdx.x -> (tensor, block within tensor) through a prefix table
constexpr int ADAM_MAXT = 48;
struct AdamMulti {
  float* p[ADAM_MAXT];
  const float* g[ADAM_MAXT];
  float* m[ADAM_MAXT];
  float* v[ADAM_MAXT];
  long n[ADAM_MAXT];
  int blk0[ADAM_MAXT + 1];
  int count;
  float* e[ADAM_MAXT];  // the averages (EMA only)
};
template <bool EMA, bool DEV, bool SCHED>
__global__ __launch_bounds__(256) void adamw_multi_kernel(AdamMulti t, AdamStep s) {
  if (!step_begin<DEV, SCHED>(s)) return;
  int k = 0;
  const int b = blockIdx.x;
  while (k + 1 < t.count && b >= t.blk0[k + 1]) ++k;
  adamw_span<EMA, false>(t.p[k], t.g[k], t.m[k], t.v[k], EMA ? t.e[k] : nullptr, s.ema_omd, nullptr, t.n[k],
                         (long)(b - t.blk0[k]) * 256 + threadIdx.x, (long)(t.blk0[k + 1] - t.blk0[k]) * 256, s.h, nullptr);
}

// SCHED: AdamSegTableD, and the step's float table from it; otherwise the float table itself
template <bool SCHED>
using SegTableArg = std::conditional_t<SCHED, AdamSegTableD, AdamSegTable>;
template <bool SCHED>
__device__ __forceinline__ AdamSegTable seg_table_now(const SegTableArg<SCHED>& t, const SchedCurrent* cur) {
  if constexpr (SCHED) return seg_table_at(t, cur->lr_factor);
  else return t;
}

template <bool EMA, bool DEV, bool SCHED>
__global__ __launch_bounds__(256) void adamw_seg_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ v, float* __restrict__ e, __bf16* __restrict__ ph, long n,
                                                        AdamStep s, SegTableArg<SCHED> t) {
  if (!step_begin<DEV, SCHED>(s)) return;
  const AdamSegTable tf = seg_table_now<SCHED>(t, s.cur);
  adamw_span<EMA, true>(p, g, m, v, e, s.ema_omd, ph, n, (long)blockIdx.x * 256 + threadIdx.x, (long)gridDim.x * 256, s.h, &tf);
}

template <bool EMA, bool DEV, bool SCHED>
__global__ __launch_bounds__(256) void adamw_planes_seg_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                               float* __restrict__ v, float* __restrict__ e, long n4, AdamStep s,
                                                               SegTableArg<SCHED> t, AdamSegs sg) {
  if (!step_begin<DEV, SCHED>(s)) return;
  const AdamSegTable tf = seg_table_now<SCHED>(t, s.cur);
  adamw_planes_span<EMA, true>(p, g, m, v, e, s.ema_omd, n4, s.h, &tf, sg);
}

// exchange of up to 48 pairs of fp32 buffers, bit for bit (the parameters against their averages): the prefix table of AdamMulti
struct SwapMulti {
  float* a[ADAM_MAXT];
  float* b[ADAM_MAXT];
  long n[ADAM_MAXT];
  int blk0[ADAM_MAXT + 1];
  int count;
};
__global__ __launch_bounds__(256) void swap_multi_kernel(SwapMulti t) {
  int k = 0;
  const int blk = blockIdx.x;
  while (k + 1 < t.count && blk >= t.blk0[k + 1]) ++k;
  float* __restrict__ a = t.a[k];
  float* __restrict__ b = t.b[k];
  const long n = t.n[k];
  const long i0 = (long)(blk - t.blk0[k]) * 256 + threadIdx.x, stride = (long)(t.blk0[k + 1] - t.blk0[k]) * 256;
  const bool vec = (((uintptr_t)a | (uintptr_t)b) & 15) == 0;
  const long n4 = vec ? (n >> 2) : 0;
  for (long i = i0; i < n4; i += stride) {
    const f32x4 A = reinterpret_cast<const f32x4*>(a)[i], B = reinterpret_cast<const f32x4*>(b)[i];
    reinterpret_cast<f32x4*>(a)[i] = B;
    reinterpret_cast<f32x4*>(b)[i] = A;
  }
  for (long i = (n4 << 2) + i0; i < n; i += stride) {
    const float A = a[i], B = b[i];
    a[i] = B;
    b[i] = A;
  }
}

// ---- bf16 gradient wire format ------------------------------------------------------------------------------
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// dst[i] = bf16(src[i]) for i < n, 0 for n <= i < npad   (npad % 8 == 0)
__global__ __launch_bounds__(256) void grad_pack_kernel(const float* __restrict__ src, __bf16* __restrict__ dst, long n, long npad) {
  const long stride = (long)gridDim.x * 256;
  for (long i8 = (long)blockIdx.x * 256 + threadIdx.x; i8 < (npad >> 3); i8 += stride) {
    const long i = i8 << 3;
    bf16x8 o;
    if (i + 8 <= n) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(src + i), b = *reinterpret_cast<const f32x4*>(src + i + 4);
      o = bf16x8{(__bf16)a.x, (__bf16)a.y, (__bf16)a.z, (__bf16)a.w, (__bf16)b.x, (__bf16)b.y, (__bf16)b.z, (__bf16)b.w};
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = (i + j < n) ? (__bf16)src[i + j] : (__bf16)0.f;
    }
    *reinterpret_cast<bf16x8*>(dst + i) = o;
  }
}

// out[c] = bf16(scale * sum_{r < W} float(recv[r * chunk + c]))  -- fp32 accumulation in rank order (deterministic)
__global__ __launch_bounds__(256) void grad_reduce_kernel(const __bf16* __restrict__ recv, __bf16* __restrict__ out, int W,
                                                         long chunk, float scale) {
  const long stride = (long)gridDim.x * 256;
  for (long i8 = (long)blockIdx.x * 256 + threadIdx.x; i8 < (chunk >> 3); i8 += stride) {
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int r = 0; r < W; ++r) {
      const bf16x8 x = *reinterpret_cast<const bf16x8*>(recv + (long)r * chunk + (i8 << 3));
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += (float)x[j];
    }
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (__bf16)(acc[j] * scale);
    *reinterpret_cast<bf16x8*>(out + (i8 << 3)) = o;
  }
}

// dst[i] = float(src[i]) for i < n
__global__ __launch_bounds__(256) void grad_unpack_kernel(const __bf16* __restrict__ src, float* __restrict__ dst, long n) {
  const long stride = (long)gridDim.x * 256;
  for (long i8 = (long)blockIdx.x * 256 + threadIdx.x; (i8 << 3) < n; i8 += stride) {
    const long i = i8 << 3;
    const bf16x8 x = *reinterpret_cast<const bf16x8*>(src + i);
    if (i + 8 <= n) {
      *reinterpret_cast<f32x4*>(dst + i) = f32x4{(float)x[0], (float)x[1], (float)x[2], (float)x[3]};
      *reinterpret_cast<f32x4*>(dst + i + 4) = f32x4{(float)x[4], (float)x[5], (float)x[6], (float)x[7]};
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (i + j < n) dst[i + j] = (float)x[j];
    }
  }
}

// ---- host side: what the launches share --------------------------------------------------------------------------------------------
static inline int stream_grid(long work_items) {
  long b = (work_items + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 256 * 8 ? 256 * 8 : b));  // up to 8 blocks per CU: enough loads in flight for HBM
}
// the grid of one buffer's update; max_blocks > 0 caps it (a BACKGROUND update, see mtvaf_adamw)
static inline int adam_grid(long n4, int max_blocks) {
  const int grid = stream_grid(n4);
  return max_blocks > 0 && max_blocks < grid ? max_blocks : grid;
}
static inline bool ema_omd_ok(float omd) { return omd >= 0.f && omd <= 1.f; }  // (false for NaN)
static inline bool sched_ptrs_ok(const void* cur, const float* clip) { return cur && !((uintptr_t)cur & 7) && !((uintptr_t)clip & 3); }
static inline const SchedCurrent* sched_cur(const void* cur) { return static_cast<const SchedCurrent*>(cur); }

// The launch selector: the instantiation <ema != NULL, clip != NULL, SCHED> of one form's kernel template.  ema and clip are the
// nullable arguments of the entry points: NULL is the form without the flag, the same body.
#define ADAMW_FORMS(K, SCHED) K<true, true, SCHED>, K<true, false, SCHED>, K<false, true, SCHED>, K<false, false, SCHED>
template <typename K, typename... A>
static inline void adamw_pick(K k_ema_dev, K k_ema, K k_dev, K k_plain, bool ema, bool dev, int grid, hipStream_t stream, A... args) {
  hipLaunchKernelGGL(ema ? (dev ? k_ema_dev : k_ema) : (dev ? k_dev : k_plain), dim3(grid), dim3(256), 0, stream, args...);
}

// the plane images of up to four matrices inside a buffer of n elements (the conditions of mtvaf_adamw_planes)
static int planes_mats(AdamSegs& sg, long n, int nmat, const long* mat_begin, const int* mat_rows, const int* mat_cols,
                       void* const* mat_img) {
  if (nmat < 0 || nmat > 4 || (nmat && (!mat_begin || !mat_rows || !mat_cols || !mat_img))) return MTVAF_ERR_ARG;
  sg = AdamSegs{};
  sg.n = nmat;
  for (int s = 0; s < nmat; ++s) {
    const long cnt = (long)mat_rows[s] * mat_cols[s];
    if (mat_rows[s] <= 0 || mat_cols[s] <= 0 || mat_cols[s] % 32 || mat_begin[s] < 0 || (mat_begin[s] & 3) || mat_begin[s] + cnt > n ||
        !mat_img[s] || (((uintptr_t)mat_img[s]) & 15))
      return MTVAF_ERR_SHAPE;
    sg.b4[s] = mat_begin[s] / 4; sg.e4[s] = (mat_begin[s] + cnt) / 4;
    sg.rows[s] = mat_rows[s]; sg.cols[s] = mat_cols[s];
    sg.img[s] = static_cast<unsigned char*>(mat_img[s]);
  }
  return MTVAF_OK;
}

// the segment table both segmented forms check before anything is launched; LR: float (AdamSegTable) or double (AdamSegTableD)
template <typename T, typename LR>
static int seg_table(T& t, long n, int nseg, const long* seg_end, const LR* seg_lr, const float* seg_wd) {
  if (n <= 0 || nseg < 1 || nseg > ADAM_MAXSEG || !seg_end || !seg_lr || !seg_wd) return MTVAF_ERR_ARG;
  long prev = 0;
  for (int k = 0; k < nseg; ++k) {
    if (seg_end[k] <= prev || (k + 1 < nseg && (seg_end[k] & 3))) return MTVAF_ERR_ARG;
    prev = seg_end[k];
  }
  if (prev != n) return MTVAF_ERR_ARG;
  if ((n + 3) / 4 >= (long)INT_MAX) return MTVAF_ERR_SHAPE;  // (the scan compares float4 indices as int)
  t.n = nseg;
  for (int k = 0; k < ADAM_MAXSEG; ++k) {
    t.end4[k] = k + 1 < nseg ? (int)(seg_end[k] / 4) : INT_MAX;
    t.lr[k] = k < nseg ? seg_lr[k] : 0;
    t.wd[k] = k < nseg ? seg_wd[k] : 0.f;
  }
  return MTVAF_OK;
}

// The prefix table of a multi-tensor call (AdamMulti, SwapMulti, SamMulti), 48 tensors per launch: fill(t, k, i) puts tensor i's
// pointers into column k, launch(t, blocks) starts the kernel; at most 1024 blocks per tensor.  The caller has checked every tensor.
template <typename T, typename Fill, typename Launch>
static int multi_launches(int count, const long* n, Fill fill, Launch launch) {
  for (int base = 0; base < count; base += ADAM_MAXT) {
    T t;
    t.count = count - base < ADAM_MAXT ? count - base : ADAM_MAXT;
    int blocks = 0;
    for (int k = 0; k < t.count; ++k) {
      const int i = base + k;
      fill(t, k, i);
      t.n[k] = n[i];
      t.blk0[k] = blocks;
      const long b = ((n[i] + 3) / 4 + 255) / 256;
      blocks += (int)(b > 1024 ? 1024 : b);
    }
    t.blk0[t.count] = blocks;
    launch(t, blocks);
    MTVAF_LAUNCH_CHECK();
  }
  return MTVAF_OK;
}
static int adamw_multi_launches(bool sched, int count, float* const* p, const float* const* g, float* const* m, float* const* v,
                                const long* n, float* const* ema, const AdamStep& s, hipStream_t stream) {
  return multi_launches<AdamMulti>(
      count, n,
      [&](AdamMulti& t, int k, int i) { t.p[k] = p[i]; t.g[k] = g[i]; t.m[k] = m[i]; t.v[k] = v[i]; t.e[k] = ema ? ema[i] : nullptr; },
      [&](const AdamMulti& t, int blocks) {
        if (sched) adamw_pick(ADAMW_FORMS(adamw_multi_kernel, true), ema != nullptr, s.clip != nullptr, blocks, stream, t, s);
        else adamw_pick(ADAMW_FORMS(adamw_multi_kernel, false), ema != nullptr, s.clip != nullptr, blocks, stream, t, s);
      });
}

// ---- the launches behind the host-scalar, _dev and _ema entry points: clip == nullptr is the host-scalar form, ema == nullptr the
// form without the average
static int adamw_launch(float* p, const float* g, float* m, float* v, long n, float lr, double beta1, double beta2, float eps,
                        float weight_decay, float bc1, float bc2_sqrt, float grad_scale, void* p_bf16, int max_blocks,
                        const float* clip, float* ema, float ema_omd, hipStream_t stream) {
  if (!p || !g || !m || !v || n <= 0) return MTVAF_ERR_ARG;
  if (ema && !ema_omd_ok(ema_omd)) return MTVAF_ERR_ARG;
  if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) & 3) return MTVAF_ERR_ALIGN;
  const AdamStep s = {make_hyper(lr, beta1, beta2, eps, weight_decay, bc1, bc2_sqrt, grad_scale), ema_omd, 0.0, nullptr, clip};
  adamw_pick(ADAMW_FORMS(adamw_flat_kernel, false), ema != nullptr, clip != nullptr, adam_grid((n + 3) / 4, max_blocks), stream,
             p, g, m, v, ema, static_cast<__bf16*>(p_bf16), n, s);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

static int adamw_planes_launch(float* p, const float* g, float* m, float* v, long n, float lr, double beta1, double beta2, float eps,
                               float weight_decay, float bc1, float bc2_sqrt, float grad_scale, int nseg, const long* seg_begin,
                               const int* seg_rows, const int* seg_cols, void* const* seg_img, int max_blocks, const float* clip,
                               float* ema, float ema_omd, hipStream_t stream) {
  if (!p || !g || !m || !v || n <= 0 || nseg < 0 || nseg > 4 || (nseg && (!seg_begin || !seg_rows || !seg_cols || !seg_img))) return MTVAF_ERR_ARG;
  if (ema && !ema_omd_ok(ema_omd)) return MTVAF_ERR_ARG;
  if ((n & 3) || (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) & 15)) return MTVAF_ERR_ALIGN;
  AdamSegs sg;
  if (const int rc = planes_mats(sg, n, nseg, seg_begin, seg_rows, seg_cols, seg_img)) return rc;
  const AdamStep s = {make_hyper(lr, beta1, beta2, eps, weight_decay, bc1, bc2_sqrt, grad_scale), ema_omd, 0.0, nullptr, clip};
  adamw_pick(ADAMW_FORMS(adamw_planes_kernel, false), ema != nullptr, clip != nullptr, adam_grid(n / 4, max_blocks), stream,
             p, g, m, v, ema, n / 4, s, sg);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

static int adamw_multi_launch(int count, float* const* p, const float* const* g, float* const* m, float* const* v, const long* n,
                              float lr, double beta1, double beta2, float eps, float weight_decay, float bc1, float bc2_sqrt,
                              float grad_scale, const float* clip, float* const* ema, float ema_omd, hipStream_t stream) {
  if (count < 0 || (count && (!p || !g || !m || !v || !n))) return MTVAF_ERR_ARG;
  if (ema && !ema_omd_ok(ema_omd)) return MTVAF_ERR_ARG;
  // every tensor is checked before the first launch: a refused call has written nothing
  for (int i = 0; i < count; ++i) {
    if (!p[i] || !g[i] || !m[i] || !v[i] || n[i] <= 0) return MTVAF_ERR_ARG;
    if (((uintptr_t)p[i] | (uintptr_t)g[i] | (uintptr_t)m[i] | (uintptr_t)v[i]) & 3) return MTVAF_ERR_ALIGN;
    if (ema && !ema[i]) return MTVAF_ERR_ARG;
    if (ema && ((uintptr_t)ema[i] & 3)) return MTVAF_ERR_ALIGN;
  }
  const AdamStep s = {make_hyper(lr, beta1, beta2, eps, weight_decay, bc1, bc2_sqrt, grad_scale), ema_omd, 0.0, nullptr, clip};
  return adamw_multi_launches(false, count, p, g, m, v, n, ema, s, stream);
}

static int swap_multi_launch(int count, float* const* a, float* const* b, const long* n, hipStream_t stream) {
  if (count < 0 || (count && (!a || !b || !n))) return MTVAF_ERR_ARG;
  // every pair is checked before the first launch: a refused call has written nothing
  for (int i = 0; i < count; ++i) {
    if (!a[i] || !b[i] || n[i] <= 0) return MTVAF_ERR_ARG;
    if (((uintptr_t)a[i] | (uintptr_t)b[i]) & 3) return MTVAF_ERR_ALIGN;
    const uintptr_t lo_a = (uintptr_t)a[i], lo_b = (uintptr_t)b[i], bytes = (uintptr_t)n[i] * 4;
    if (lo_a < lo_b + bytes && lo_b < lo_a + bytes) return MTVAF_ERR_ARG;  // the two sides of a pair overlap
  }
  return multi_launches<SwapMulti>(
      count, n, [&](SwapMulti& t, int k, int i) { t.a[k] = a[i]; t.b[k] = b[i]; },
      [&](const SwapMulti& t, int blocks) { hipLaunchKernelGGL(swap_multi_kernel, dim3(blocks), dim3(256), 0, stream, t); });
}

// ---- sharpness-aware minimisation: the ascent step in weight space and the way back (mtvaf_sam_*; mtvaf_amd/optim.py) --
// sam_state = {norm, scale, finite, 0} is written by mtvaf_sam_finalize (csrc/gradnorm.hip) from the partial sums of
// mtvaf_grad_sqnorm_multi.  Per element
//     perturb:  backup = p;  p = fmaf(scale, g, p)          12 B read and written per parameter, + 2 B shadow or 6 B plane images
//     restore:  p = backup                                    8 B
// fmaf is ONE correctly rounded operation, so the vector body, the scalar body, the plane form and the multi-tensor form give the
// same bits.  finite == 0 (block-uniform): p is carried over unchanged -- no arithmetic touches it, an inf or NaN in g cannot reach
// it -- while backup, the bf16 shadow and the plane images are still written, from that unchanged p: after either outcome backup
// holds the weights to return to and every image matches p, so the caller stamps them fresh without knowing which one it was.
// RESTORE: g and the state are not read.
template <bool RESTORE>
__device__ __forceinline__ f32x4 sam_vec4(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ backup, long i,
                                          float scale, bool apply) {
  f32x4 P;
  if constexpr (RESTORE) {
    P = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(backup) + i);  // (the backup is read once and never again)
  } else {
    P = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p) + i);
    __builtin_nontemporal_store(P, reinterpret_cast<f32x4*>(backup) + i);
    if (apply) {
      const f32x4 G = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(g) + i);
#pragma unroll
      for (int j = 0; j < 4; ++j) P[j] = fmaf(scale, G[j], P[j]);
    }
  }
  reinterpret_cast<f32x4*>(p)[i] = P;  // (read again by the next forward pass)
  return P;
}

template <bool RESTORE>
__device__ __forceinline__ void sam_span(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ backup,
                                         __bf16* __restrict__ ph, long n, long i0, long stride, float scale, bool apply) {
  // vector body on 16-byte bases, scalar otherwise and for the tail: as adamw_span
  const bool vec = ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)backup) & 15) == 0) && (!ph || ((uintptr_t)ph & 7) == 0);
  const long n4 = vec ? (n >> 2) : 0;
  for (long i = i0; i < n4; i += stride) {
    const f32x4 P = sam_vec4<RESTORE>(p, g, backup, i, scale, apply);
    if (ph) reinterpret_cast<bf16x4*>(ph)[i] = to_bf16x4(P);
  }
  for (long i = (n4 << 2) + i0; i < n; i += stride) {
    float P;
    if constexpr (RESTORE) {
      P = backup[i];
    } else {
      P = p[i];
      backup[i] = P;
      if (apply) P = fmaf(scale, g[i], P);
    }
    p[i] = P;
    if (ph) ph[i] = (__bf16)P;
  }
}

// the state's two words a perturb launch reads (block-uniform, two scalar loads)
__device__ __forceinline__ void sam_read(const float* __restrict__ state, float& scale, bool& apply) {
  scale = state[1];
  apply = state[2] != 0.f;
}

template <bool RESTORE>
__global__ __launch_bounds__(256) void sam_kernel(float* p, const float* g, float* backup, __bf16* ph, long n, const float* state) {
  float scale = 0.f;
  bool apply = false;
  if constexpr (!RESTORE) sam_read(state, scale, apply);
  sam_span<RESTORE>(p, g, backup, ph, n, (long)blockIdx.x * 256 + threadIdx.x, (long)gridDim.x * 256, scale, apply);
}

template <bool RESTORE>
__global__ __launch_bounds__(256) void sam_planes_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ backup,
                                                         long n4, AdamSegs sg, const float* __restrict__ state) {
  float scale = 0.f;
  bool apply = false;
  if constexpr (!RESTORE) sam_read(state, scale, apply);
  const long stride = (long)gridDim.x * 256;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) mats_store4(sg, i, sam_vec4<RESTORE>(p, g, backup, i, scale,
       apply));
}

struct SamMulti {  // the prefix table of AdamMulti
  float* p[ADAM_MAXT];
  const float* g[ADAM_MAXT];
  float* b[ADAM_MAXT];
  long n[ADAM_MAXT];
  int blk0[ADAM_MAXT + 1];
  int count;
};
template <bool RESTORE>
__global__ __launch_bounds__(256) void sam_multi_kernel(SamMulti t, const float* state) {
  float scale = 0.f;
  bool apply = false;
  if constexpr (!RESTORE) sam_read(state, scale, apply);
  int k = 0;
  const int blk = blockIdx.x;
  while (k + 1 < t.count && blk >= t.blk0[k + 1]) ++k;
  sam_span<RESTORE>(t.p[k], t.g[k], t.b[k], nullptr, t.n[k], (long)(blk - t.blk0[k]) * 256 + threadIdx.x,
                    (long)(t.blk0[k + 1] - t.blk0[k]) * 256, scale, apply);
}

static inline bool ranges_overlap(const void* a, const void* b, long n) {
  const uintptr_t lo_a = (uintptr_t)a, lo_b = (uintptr_t)b, bytes = (uintptr_t)n * 4;
  return lo_a < lo_b + bytes && lo_b < lo_a + bytes;
}

// what every mtvaf_sam_* form checks of one (p, g, backup) triple; g == nullptr with restore.  The family reports a misaligned
// pointer as MTVAF_ERR_ARG too (include/mtvaf_hip.h)
static inline bool sam_triple_ok(const float* p, const float* g, const float* backup, long n, bool restore, uintptr_t align_mask) {
  if (!p || !backup || (!restore && !g) || n <= 0) return false;
  if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)backup) & align_mask) return false;
  if (ranges_overlap(p, backup, n) || (!restore && (ranges_overlap(g, backup, n) || ranges_overlap(g, p, n)))) return false;
  return true;
}

static int sam_launch(float* p, const float* g, float* backup, long n, const float* state, void* p_bf16, bool restore,
                      hipStream_t stream) {
  if (!sam_triple_ok(p, g, backup, n, restore, 3) || (!restore && (!state || ((uintptr_t)state & 3))) || ((uintptr_t)p_bf16 & 1))
    return MTVAF_ERR_ARG;
  const int grid = stream_grid((n + 3) / 4);
  hipLaunchKernelGGL(restore ? sam_kernel<true> : sam_kernel<false>, dim3(grid), dim3(256), 0, stream, p, g, backup,
                     static_cast<__bf16*>(p_bf16), n, state);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

static int sam_planes_launch(float* p, const float* g, float* backup, long n, const float* state, int nmat, const long* mat_begin,
                             const int* mat_rows, const int* mat_cols, void* const* mat_img, bool restore, hipStream_t stream) {
  if (!sam_triple_ok(p, g, backup, n, restore, 15) || (n & 3) || (!restore && (!state || ((uintptr_t)state & 3)))) return MTVAF_ERR_ARG;
  AdamSegs sg;
  if (const int rc = planes_mats(sg, n, nmat, mat_begin, mat_rows, mat_cols, mat_img)) return rc;
  hipLaunchKernelGGL(restore ? sam_planes_kernel<true> : sam_planes_kernel<false>, dim3(stream_grid(n / 4)), dim3(256), 0, stream, p, g,
                     backup, n / 4, sg, state);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

static int sam_multi_launch(int count, float* const* p, const float* const* g, float* const* backup, const long* n, const float* state,
                            bool restore, hipStream_t stream) {
  if (count < 0 || (count && (!p || !backup || !n || (!restore && !g))) || (!restore && (!state || ((uintptr_t)state & 3))))
    return MTVAF_ERR_ARG;
  // every tensor is checked before the first launch: a refused call has written nothing
  for (int i = 0; i < count; ++i)
    if (!sam_triple_ok(p[i], restore ? nullptr : g[i], backup[i], n[i], restore, 3)) return MTVAF_ERR_ARG;
  return multi_launches<SamMulti>(
      count, n, [&](SamMulti& t, int k, int i) { t.p[k] = p[i]; t.g[k] = restore ? nullptr : g[i]; t.b[k] = backup[i]; },
      [&](const SamMulti& t, int blocks) {
        hipLaunchKernelGGL(restore ? sam_multi_kernel<true> : sam_multi_kernel<false>, dim3(blocks), dim3(256), 0, stream, t, state);
      });
}

}  // namespace mtvaf

using namespace mtvaf;

extern "C" {

// One flat tensor (an encoder layer's parameter buffer).  bias corrections are passed in: bc1 = 1 - beta1^t,
// bc2_sqrt = sqrt(1 - beta2^t).  p_bf16 (optional) receives the updated parameter rounded to bf16.
// max_blocks > 0 caps the grid: a BACKGROUND update.  At full width (2048 blocks) the update streams at the HBM rate
// (6.3 TB/s) and starves the operand fetches of the MFMA-bound products it runs beside for its 32 us; 128 blocks trickle
// at ~1 TB/s under them instead (measured per step, same box: fp32 bs 32 18.95 -> 18.70 ms, bf16 bs 64 11.78 -> 11.56;
// 64 blocks and fewer take longer than the layer's backward pass they hide behind and lose).  0: full width.
int mtvaf_adamw(float* p, const float* g, float* m, float* v, long n, float lr, double beta1, double beta2, float eps,
                float weight_decay, float bc1, float bc2_sqrt, float grad_scale, void* p_bf16, int max_blocks,
                hipStream_t stream) {
  return adamw_launch(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, bc1, bc2_sqrt, grad_scale, p_bf16, max_blocks, nullptr,
                      nullptr, 0.f, stream);
}

// mtvaf_adamw with the gradient scaled by grad_scale * clip_state[1] on the device; clip_state[2] == 0: nothing is written.
int mtvaf_adamw_dev(float* p, const float* g, float* m, float* v, long n, float lr, double beta1, double beta2, float eps,
                    float weight_decay, float bc1, float bc2_sqrt, float grad_scale, void* p_bf16, int max_blocks,
                    const float* clip_state, hipStream_t stream) {
  if (!clip_state) return MTVAF_ERR_ARG;
  if ((uintptr_t)clip_state & 3) return MTVAF_ERR_ALIGN;
  return adamw_launch(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, bc1, bc2_sqrt, grad_scale, p_bf16, max_blocks, clip_state,
                      nullptr, 0.f, stream);
}

// mtvaf_adamw over a flat buffer (n % 4 == 0, 16-byte aligned) that also rewrites the plane images of nseg <= 4 row-major fp32
// matrices inside it: matrix s starts at element seg_begin[s] (% 4 == 0) of the buffer, is [seg_rows[s]][seg_cols[s]] (cols % 32 == 0)
// and has its tile-blocked image (6 bytes per element) at seg_img[s].  Same update as mtvaf_adamw, bit for bit.
int mtvaf_adamw_planes(float* p, const float* g, float* m, float* v, long n, float lr, double beta1, double beta2, float eps,
                       float weight_decay, float bc1, float bc2_sqrt, float grad_scale, int nseg, const long* seg_begin,
                       const int* seg_rows, const int* seg_cols, void* const* seg_img, int max_blocks, hipStream_t stream) {
  return adamw_planes_launch(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, bc1, bc2_sqrt, grad_scale, nseg, seg_begin, seg_rows,
                             seg_cols, seg_img, max_blocks, nullptr, nullptr, 0.f, stream);
}

// mtvaf_adamw_planes under a device clip state: with clip_state[2] == 0 the plane images keep their bits too.
int mtvaf_adamw_planes_dev(float* p, const float* g, float* m, float* v, long n, float lr, double beta1, double beta2, float eps,
                           float weight_decay, float bc1, float bc2_sqrt, float grad_scale, int nseg, const long* seg_begin,
                           const int* seg_rows, const int* seg_cols, void* const* seg_img, int max_blocks, const float* clip_state,
                           hipStream_t stream) {
  if (!clip_state) return MTVAF_ERR_ARG;
  if ((uintptr_t)clip_state & 3) return MTVAF_ERR_ALIGN;
  return adamw_planes_launch(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, bc1, bc2_sqrt, grad_scale, nseg, seg_begin, seg_rows,
                             seg_cols, seg_img, max_blocks, clip_state, nullptr, 0.f, stream);
}

// `count` tensors sharing one set of hyper-parameters (a torch parameter group); host arrays of device pointers.  Every tensor is
// checked before the first launch: a refused call has written nothing.
int mtvaf_adamw_multi(int count, float* const* p, const float* const* g, float* const* m, float* const* v, const long* n,
                      float lr, double beta1, double beta2, float eps, float weight_decay, float bc1, float bc2_sqrt,
                      float grad_scale, hipStream_t stream) {
  return adamw_multi_launch(count, p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, bc1, bc2_sqrt, grad_scale, nullptr, nullptr, 0.f,
                            stream);
}

int mtvaf_adamw_multi_dev(int count, float* const* p, const float* const* g, float* const* m, float* const* v, const long* n,
                          float lr, double beta1, double beta2, float eps, float weight_decay, float bc1, float bc2_sqrt,
                          float grad_scale, const float* clip_state, hipStream_t stream) {
  if (!clip_state) return MTVAF_ERR_ARG;
  if ((uintptr_t)clip_state & 3) return MTVAF_ERR_ALIGN;
  return adamw_multi_launch(count, p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, bc1, bc2_sqrt, grad_scale, clip_state, nullptr,
                            0.f, stream);
}

// The three updates with an exponential moving average of the parameters kept in the same pass (the EMA flag at the head of this
// file): ema / ema[i] as long as p / p[i] and not NULL, ema_omd = 1 - decay in [0, 1] (1: the average becomes the new parameter
// exactly).  clip_state NULL: the host-scalar form; otherwise the *_dev form -- with clip_state[2] == 0 the average keeps its bits
// like everything else.
int mtvaf_adamw_ema(float* p, const float* g, float* m, float* v, long n, float lr, double beta1, double beta2, float eps,
                    float weight_decay, float bc1, float bc2_sqrt, float grad_scale, void* p_bf16, int max_blocks, float* ema,
                    float ema_omd, const float* clip_state, hipStream_t stream) {
  if ((uintptr_t)clip_state & 3) return MTVAF_ERR_ALIGN;
  if (!ema) return MTVAF_ERR_ARG;
  return adamw_launch(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, bc1, bc2_sqrt, grad_scale, p_bf16, max_blocks, clip_state, ema,
                      ema_omd, stream);
}

int mtvaf_adamw_planes_ema(float* p, const float* g, float* m, float* v, long n, float lr, double beta1, double beta2, float eps,
                           float weight_decay, float bc1, float bc2_sqrt, float grad_scale, int nseg, const long* seg_begin,
                           const int* seg_rows, const int* seg_cols, void* const* seg_img, int max_blocks, float* ema, float ema_omd,
                           const float* clip_state, hipStream_t stream) {
  if ((uintptr_t)clip_state & 3) return MTVAF_ERR_ALIGN;
  if (!ema) return MTVAF_ERR_ARG;
  return adamw_planes_launch(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, bc1, bc2_sqrt, grad_scale, nseg, seg_begin, seg_rows,
                             seg_cols, seg_img, max_blocks, clip_state, ema, ema_omd, stream);
}

int mtvaf_adamw_multi_ema(int count, float* const* p, const float* const* g, float* const* m, float* const* v, const long* n,
                          float lr, double beta1, double beta2, float eps, float weight_decay, float bc1, float bc2_sqrt,
                          float grad_scale, float* const* ema, float ema_omd, const float* clip_state, hipStream_t stream) {
  if ((uintptr_t)clip_state & 3) return MTVAF_ERR_ALIGN;
  if ((count > 0 && !ema) || !ema_omd_ok(ema_omd)) return MTVAF_ERR_ARG;
  return adamw_multi_launch(count, p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, bc1, bc2_sqrt, grad_scale, clip_state, ema,
                            ema_omd, stream);
}

// mtvaf_adamw / mtvaf_adamw_planes with lr and weight decay per segment of the buffer (the head of the segment table above);
// clip_state, ema and p_bf16 are nullable arguments: one entry point each instead of a _dev / _ema family.
int mtvaf_adamw_seg(float* p, const float* g, float* m, float* v, long n, int nseg, const long* seg_end, const float* seg_lr,
                    const float* seg_wd, double beta1, double beta2, float eps, float bc1, float bc2_sqrt, float grad_scale,
                    void* p_bf16, int max_blocks, float* ema, float ema_omd, const float* clip_state, hipStream_t stream) {
  if (!p || !g || !m || !v) return MTVAF_ERR_ARG;
  if (ema && !ema_omd_ok(ema_omd)) return MTVAF_ERR_ARG;
  AdamSegTable t;
  if (const int rc = seg_table(t, n, nseg, seg_end, seg_lr, seg_wd)) return rc;
  if ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) & 15) || ((uintptr_t)p_bf16 & 7) || ((uintptr_t)clip_state & 3))
    return MTVAF_ERR_ALIGN;
  // (lr, wd: per segment, from the table)
  const AdamStep s = {make_hyper(0.f, beta1, beta2, eps, 0.f, bc1, bc2_sqrt, grad_scale), ema_omd, 0.0, nullptr, clip_state};
  adamw_pick(ADAMW_FORMS(adamw_seg_kernel, false), ema != nullptr, clip_state != nullptr, adam_grid((n + 3) / 4, max_blocks), stream,
             p, g, m, v, ema, static_cast<__bf16*>(p_bf16), n, s, t);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

int mtvaf_adamw_planes_seg(float* p, const float* g, float* m, float* v, long n, int nseg, const long* seg_end, const float* seg_lr,
                           const float* seg_wd, double beta1, double beta2, float eps, float bc1, float bc2_sqrt, float grad_scale,
                           int nmat, const long* mat_begin, const int* mat_rows, const int* mat_cols, void* const* mat_img,
                           int max_blocks, float* ema, float ema_omd, const float* clip_state, hipStream_t stream) {
  if (!p || !g || !m || !v || nmat < 0 || nmat > 4 || (nmat && (!mat_begin || !mat_rows || !mat_cols || !mat_img))) return MTVAF_ERR_ARG;
  if (ema && !ema_omd_ok(ema_omd)) return MTVAF_ERR_ARG;
  AdamSegTable t;
  if (const int rc = seg_table(t, n, nseg, seg_end, seg_lr, seg_wd)) return rc;
  if ((n & 3) || (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) & 15) || ((uintptr_t)clip_state & 3))
    return MTVAF_ERR_ALIGN;
  AdamSegs sg;
  if (const int rc = planes_mats(sg, n, nmat, mat_begin, mat_rows, mat_cols, mat_img)) return rc;
  const AdamStep s = {make_hyper(0.f, beta1, beta2, eps, 0.f, bc1, bc2_sqrt, grad_scale), ema_omd, 0.0, nullptr, clip_state};
  adamw_pick(ADAMW_FORMS(adamw_planes_seg_kernel, false), ema != nullptr, clip_state != nullptr, adam_grid(n / 4, max_blocks), stream,
             p, g, m, v, ema, n / 4, s, t, sg);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

// ++*counter (device int64) and the table's row for that step -> current (32 bytes, 8-byte aligned); rows of 24 bytes.  One block.
int mtvaf_adamw_sched_advance(const void* table, long rows, long* counter, void* current, hipStream_t stream) {
  if (!table || rows < 1 || !counter || !current) return MTVAF_ERR_ARG;
  if (((uintptr_t)table | (uintptr_t)counter | (uintptr_t)current) & 7) return MTVAF_ERR_ALIGN;
  hipLaunchKernelGGL(sched_advance_kernel, dim3(1), dim3(64), 0, stream, static_cast<const SchedRow*>(table), rows, counter,
                     static_cast<SchedCurrent*>(current));
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

// The five updates with lr = (float)(base_lr * current.lr_factor) and bc1, bc2_sqrt, ema_omd read from `current` (the SCHED flag);
// ema, clip_state (and p_bf16) nullable as in mtvaf_adamw_seg.  current.overrun != 0: nothing is written.
int mtvaf_adamw_sched(float* p, const float* g, float* m, float* v, long n, double base_lr, double beta1, double beta2, float eps,
                      float weight_decay, float grad_scale, void* p_bf16, int max_blocks, float* ema, const float* clip_state,
                      const void* current, hipStream_t stream) {
  if (!p || !g || !m || !v || n <= 0 || !current) return MTVAF_ERR_ARG;
  if ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) & 3) || !sched_ptrs_ok(current,
      clip_state)) return MTVAF_ERR_ALIGN;
  const AdamStep s = {make_hyper(0.f, beta1, beta2, eps, weight_decay, 1.f, 1.f, grad_scale), 0.f, base_lr, sched_cur(current), clip_state};
  adamw_pick(ADAMW_FORMS(adamw_flat_kernel, true), ema != nullptr, clip_state != nullptr, adam_grid((n + 3) / 4, max_blocks), stream,
             p, g, m, v, ema, static_cast<__bf16*>(p_bf16), n, s);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

int mtvaf_adamw_planes_sched(float* p, const float* g, float* m, float* v, long n, double base_lr, double beta1, double beta2,
                             float eps, float weight_decay, float grad_scale, int nmat, const long* mat_begin, const int* mat_rows,
                             const int* mat_cols, void* const* mat_img, int max_blocks, float* ema, const float* clip_state,
                             const void* current, hipStream_t stream) {
  if (!p || !g || !m || !v || n <= 0 || !current) return MTVAF_ERR_ARG;
  if ((n & 3) || (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) & 15) || !sched_ptrs_ok(current, clip_state))
    return MTVAF_ERR_ALIGN;
  AdamSegs sg;
  if (const int rc = planes_mats(sg, n, nmat, mat_begin, mat_rows, mat_cols, mat_img)) return rc;
  const AdamStep s = {make_hyper(0.f, beta1, beta2, eps, weight_decay, 1.f, 1.f, grad_scale), 0.f, base_lr, sched_cur(current), clip_state};
  adamw_pick(ADAMW_FORMS(adamw_planes_kernel, true), ema != nullptr, clip_state != nullptr, adam_grid(n / 4, max_blocks), stream,
             p, g, m, v, ema, n / 4, s, sg);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

int mtvaf_adamw_multi_sched(int count, float* const* p, const float* const* g, float* const* m, float* const* v, const long* n,
                            double base_lr, double beta1, double beta2, float eps, float weight_decay, float grad_scale,
                            float* const* ema, const float* clip_state, const void* current, hipStream_t stream) {
  if (count < 0 || (count && (!p || !g || !m || !v || !n)) || !current) return MTVAF_ERR_ARG;
  if (!sched_ptrs_ok(current, clip_state)) return MTVAF_ERR_ALIGN;
  // every tensor is checked before the first launch: a refused call has written nothing
  for (int i = 0; i < count; ++i) {
    if (!p[i] || !g[i] || !m[i] || !v[i] || n[i] <= 0 || (ema && !ema[i])) return MTVAF_ERR_ARG;
    if (((uintptr_t)p[i] | (uintptr_t)g[i] | (uintptr_t)m[i] | (uintptr_t)v[i] | (uintptr_t)(ema ? ema[i] : nullptr)) & 3) return MTVAF_ERR_ALIGN;
  }
  const AdamStep s = {make_hyper(0.f, beta1, beta2, eps, weight_decay, 1.f, 1.f, grad_scale), 0.f, base_lr, sched_cur(current), clip_state};
  return adamw_multi_launches(true, count, p, g, m, v, n, ema, s, stream);
}

int mtvaf_adamw_seg_sched(float* p, const float* g, float* m, float* v, long n, int nseg, const long* seg_end, const double* seg_lr,
                          const float* seg_wd, double beta1, double beta2, float eps, float grad_scale, void* p_bf16, int max_blocks,
                          float* ema, const float* clip_state, const void* current, hipStream_t stream) {
  if (!p || !g || !m || !v || !current) return MTVAF_ERR_ARG;
  AdamSegTableD td;
  if (const int rc = seg_table(td, n, nseg, seg_end, seg_lr, seg_wd)) return rc;
  if ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) & 15) || ((uintptr_t)p_bf16 & 7) || !sched_ptrs_ok(current, clip_state))
    return MTVAF_ERR_ALIGN;
  const AdamStep s = {make_hyper(0.f, beta1, beta2, eps, 0.f, 1.f, 1.f, grad_scale), 0.f, 0.0, sched_cur(current), clip_state};
  adamw_pick(ADAMW_FORMS(adamw_seg_kernel, true), ema != nullptr, clip_state != nullptr, adam_grid((n + 3) / 4, max_blocks), stream,
             p, g, m, v, ema, static_cast<__bf16*>(p_bf16), n, s, td);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

int mtvaf_adamw_planes_seg_sched(float* p, const float* g, float* m, float* v, long n, int nseg, const long* seg_end,
                                 const double* seg_lr, const float* seg_wd, double beta1, double beta2, float eps, float grad_scale,
                                 int nmat, const long* mat_begin, const int* mat_rows, const int* mat_cols, void* const* mat_img,
                                 int max_blocks, float* ema, const float* clip_state, const void* current, hipStream_t stream) {
  if (!p || !g || !m || !v || !current) return MTVAF_ERR_ARG;
  AdamSegTableD td;
  if (const int rc = seg_table(td, n, nseg, seg_end, seg_lr, seg_wd)) return rc;
  if ((n & 3) || (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) & 15) || !sched_ptrs_ok(current, clip_state))
    return MTVAF_ERR_ALIGN;
  AdamSegs sg;
  if (const int rc = planes_mats(sg, n, nmat, mat_begin, mat_rows, mat_cols, mat_img)) return rc;
  const AdamStep s = {make_hyper(0.f, beta1, beta2, eps, 0.f, 1.f, 1.f, grad_scale), 0.f, 0.0, sched_cur(current), clip_state};
  adamw_pick(ADAMW_FORMS(adamw_planes_seg_kernel, true), ema != nullptr, clip_state != nullptr, adam_grid(n / 4, max_blocks), stream,
             p, g, m, v, ema, n / 4, s, td, sg);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

// a[i] <-> b[i], n[i] floats each, bit for bit; host arrays of device pointers, any count (48 pairs per launch).  A pair whose two
// sides overlap is refused before anything is launched.
int mtvaf_swap_f32_multi(int count, float* const* a, float* const* b, const long* n, hipStream_t stream) {
  return swap_multi_launch(count, a, b, n, stream);
}

// The SAM ascent step under the device state of mtvaf_sam_finalize: backup = p, p = fmaf(sam_state[1], g, p); with sam_state[2] == 0
// p keeps its bits and backup, the shadow and the images are written from it (the head of the sam kernels above).  The restore forms
// copy backup over p and rewrite the shadow / the images from it.  Any bad argument: MTVAF_ERR_ARG (matrix tables: as
// mtvaf_adamw_planes), nothing launched.
int mtvaf_sam_perturb(float* p, const float* g, float* backup, long n, const float* sam_state, void* p_bf16, hipStream_t stream) {
  return sam_launch(p, g, backup, n, sam_state, p_bf16, false, stream);
}

int mtvaf_sam_perturb_planes(float* p, const float* g, float* backup, long n, const float* sam_state, int nseg, const long* seg_begin,
                             const int* seg_rows, const int* seg_cols, void* const* seg_img, hipStream_t stream) {
  return sam_planes_launch(p, g, backup, n, sam_state, nseg, seg_begin, seg_rows, seg_cols, seg_img, false, stream);
}

int mtvaf_sam_perturb_multi(int count, float* const* p, const float* const* g, float* const* backup, const long* n,
                            const float* sam_state, hipStream_t stream) {
  return sam_multi_launch(count, p, g, backup, n, sam_state, false, stream);
}

int mtvaf_sam_restore(float* p, const float* backup, long n, void* p_bf16, hipStream_t stream) {
  return sam_launch(p, nullptr, const_cast<float*>(backup), n, nullptr, p_bf16, true, stream);
}

int mtvaf_sam_restore_planes(float* p, const float* backup, long n, int nseg, const long* seg_begin, const int* seg_rows,
                             const int* seg_cols, void* const* seg_img, hipStream_t stream) {
  return sam_planes_launch(p, nullptr, const_cast<float*>(backup), n, nullptr, nseg, seg_begin, seg_rows, seg_cols, seg_img, true, stream);
}

int mtvaf_sam_restore_multi(int count, float* const* p, const float* const* backup, const long* n, hipStream_t stream) {
  return sam_multi_launch(count, p, nullptr, const_cast<float* const*>(backup), n, nullptr, true, stream);
}

int mtvaf_grad_pack_bf16(const float* src, void* dst, long n, long npad, hipStream_t stream) {
  if (!src || !dst || n <= 0 || npad < n || (npad & 7)) return MTVAF_ERR_ARG;
  if (((uintptr_t)src | (uintptr_t)dst) & 15) return MTVAF_ERR_ALIGN;
  hipLaunchKernelGGL(grad_pack_kernel, dim3(stream_grid(npad / 8)), dim3(256), 0, stream, src, static_cast<__bf16*>(dst), n, npad);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

int mtvaf_grad_reduce_bf16(const void* recv, void* out, int world, long chunk, float scale, hipStream_t stream) {
  if (!recv || !out || world <= 0 || chunk <= 0 || (chunk & 7)) return MTVAF_ERR_ARG;
  if (((uintptr_t)recv | (uintptr_t)out) & 15) return MTVAF_ERR_ALIGN;
  hipLaunchKernelGGL(grad_reduce_kernel, dim3(stream_grid(chunk / 8)), dim3(256), 0, stream, static_cast<const __bf16*>(recv),
                     static_cast<__bf16*>(out), world, chunk, scale);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

int mtvaf_grad_unpack_bf16(const void* src, float* dst, long n, hipStream_t stream) {
  if (!src || !dst || n <= 0) return MTVAF_ERR_ARG;
  if (((uintptr_t)src | (uintptr_t)dst) & 15) return MTVAF_ERR_ALIGN;
  hipLaunchKernelGGL(grad_unpack_kernel, dim3(stream_grid((n + 7) / 8)), dim3(256), 0, stream, static_cast<const __bf16*>(src), dst, n);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

}  // extern "C"
