// Global gradient norm for clipping inside the AdamW step (mtvaf_amd/optim.py; the reference trainer does not clip,
// modules/train.py:620-625 -- new functionality).  Two launches, no atomics, no host synchronisation:
//
//   grad_sqnorm_kernel   every tensor is cut into chunks of SQ_CHUNK elements (a compile-time number: the cut depends on the
//                        lengths alone, never on the grid or the device); ONE block per chunk writes the chunk's sum of squares
//                        to its own slot of a double workspace.  Squares and sums are double from the first operation: a
//                        gradient of 1e20 squares to 1e40, and the error of the sum (n * 2^-53) stays far below the one rounding
//                        to fp32 at the end for any length.
//   grad_clip_finalize   one block adds the slots in index order and writes {norm, coef, finite, 0} for the *_dev updates of
//                        csrc/optim.hip:  coef = min(1, max_norm / (norm + 1e-6))  (torch.nn.utils.clip_grad_norm_).
//
// Order of every addition is fixed by (lengths, 16-byte alignment of the pointers): same inputs, same bits.
// The kernel reads 4 B per element once; per element it spends one conversion and one fp64 FMA.
#include "common.h"

namespace mtvaf {

constexpr long SQ_CHUNK = 65536;  // elements per block: 64 float4 per lane
constexpr int SQ_MAXT = 48;       // tensors per launch (as ADAM_MAXT: the table travels in the kernel arguments)

struct SqMulti {
  const float* g[SQ_MAXT];
  long n[SQ_MAXT];
  int blk0[SQ_MAXT + 1];  // first block (= first chunk) of tensor k within this launch
  int count;
};

static inline long sq_chunks(long n) { return (n + SQ_CHUNK - 1) / SQ_CHUNK; }

// sum over the 256 lanes of the block, in a fixed order: butterfly inside each wave, then the four wave sums in wave order
__device__ __forceinline__ double block_sum_256(double x, double* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = x;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

__global__ __launch_bounds__(256) void grad_sqnorm_kernel(SqMulti t, double* __restrict__ part) {
  __shared__ double sh[4];
  int k = 0;
  const int b = blockIdx.x;
  while (k + 1 < t.count && b >= t.blk0[k + 1]) ++k;
  const long c0 = (long)(b - t.blk0[k]) * SQ_CHUNK;
  const long n = (t.n[k] - c0 < SQ_CHUNK) ? t.n[k] - c0 : SQ_CHUNK;  // >= 1: the host made ceil(n / SQ_CHUNK) blocks
  const float* __restrict__ g = t.g[k] + c0;  // (c0 * 4 is a multiple of 16: a chunk is aligned as its tensor is)
  // vector body when the base is 16-byte aligned (views into packed storage may be 4-byte aligned only), scalar otherwise and
  // for the tail -- as adamw_span (csrc/optim.hip)
  const long n4 = (((uintptr_t)g & 15) == 0) ? (n >> 2) : 0;
  const f32x4* __restrict__ g4 = reinterpret_cast<const f32x4*>(g);
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  long i = threadIdx.x;
  for (; i + 768 < n4; i += 1024) {  // four loads in flight per lane
    const f32x4 x0 = g4[i], x1 = g4[i + 256];
    const f32x4 x2 = g4[i + 512], x3 = g4[i + 768];
    const f32x4 xs[4] = {x0, x1, x2, x3};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const double d0 = (double)xs[u].x, d1 = (double)xs[u].y, d2 = (double)xs[u].z, d3 = (double)xs[u].w;
      a0 = fma(d0, d0, a0); a1 = fma(d1, d1, a1); a2 = fma(d2, d2, a2); a3 = fma(d3, d3, a3);
    }
  }
  for (; i < n4; i += 256) {
    const f32x4 x = g4[i];
    const double d0 = (double)x.x, d1 = (double)x.y, d2 = (double)x.z, d3 = (double)x.w;
    a0 = fma(d0, d0, a0); a1 = fma(d1, d1, a1); a2 = fma(d2, d2, a2); a3 = fma(d3, d3, a3);
  }
  for (long j = (n4 << 2) + threadIdx.x; j < n; j += 256) {
    const double d = (double)g[j];
    a0 = fma(d, d, a0);
  }
  const double s = block_sum_256((a0 + a1) + (a2 + a3), sh);
  if (threadIdx.x == 0) part[b] = s;
}

// one block of 256 lanes: the `count` slots added in index order -> lane 0's return value (the other lanes': 0)
__device__ __forceinline__ double ordered_sum_256(const double* __restrict__ part, long count, double* sh) {
  double sum = 0.0;  // (lane 0's)
  for (long base = 0; base < count; base += 256) {
    const long i = base + threadIdx.x;
    sh[threadIdx.x] = i < count ? part[i] : 0.0;  // one coalesced load per 256 slots ...
    __syncthreads();
    if (threadIdx.x == 0) {
      const int m = count - base < 256 ? (int)(count - base) : 256;
      for (int j = 0; j < m; j += 8) {  // ... added in index order, eight LDS reads ahead of the chain of additions
        double x[8];                    // (slots past `count` hold 0.0: adding them changes nothing)
#pragma unroll
        for (int u = 0; u < 8; ++u) x[u] = sh[j + u];
#pragma unroll
        for (int u = 0; u < 8; ++u) sum += x[u];
      }
    }
    __syncthreads();
  }
  return sum;
}

// state = {norm, coef, finite (1.f / 0.f), 0.f}.  `finite` is the *_dev kernels' permission to write: with skip_nonfinite == 0
// it is always 1 and a non-finite norm reaches the update through coef as it does in torch (inf -> 0, NaN -> NaN).
__global__ __launch_bounds__(256) void grad_clip_finalize_kernel(const double* __restrict__ part, long count, float max_norm,
                                                                 int skip_nonfinite, float* __restrict__ state,
                                                                 int* __restrict__ skipped) {
  __shared__ double sh[256];
  const double sum = ordered_sum_256(part, count, sh);
  if (threadIdx.x != 0) return;
  const double nd = sqrt(sum);
  const float norm = (float)nd;
  // a norm that fp32 cannot hold counts as non-finite: the coefficient could not be formed from it
  const bool finite = (norm - norm) == 0.f;
  float coef = 1.f;
  if (max_norm > 0.f) {
    const float c = (float)((double)max_norm / (nd + 1e-6));
    coef = c < 1.f ? c : (c != c ? c : 1.f);  // clamp(max = 1) that lets NaN through, as torch's does
  }
  if (!finite && skip_nonfinite) coef = 0.f;
  state[0] = norm;
  state[1] = coef;
  state[2] = (finite || !skip_nonfinite) ? 1.f : 0.f;
  state[3] = 0.f;
  if (!finite && skip_nonfinite && skipped) *skipped += 1;
}

// The same sum for the SAM ascent step (mtvaf_sam_perturb*, csrc/optim.hip): state = {norm, scale, finite, 0.f} with
// scale = (float)(rho / (norm + 1e-12)), quotient and sum in double, ONE rounding.  A norm that fp32 cannot hold: scale = 0,
// finite = 0 -- the perturb launches then leave the parameters alone -- and *skipped += 1.
__global__ __launch_bounds__(256) void sam_finalize_kernel(const double* __restrict__ part, long count, float rho,
                                                           float* __restrict__ state, int* __restrict__ skipped) {
  __shared__ double sh[256];
  const double sum = ordered_sum_256(part, count, sh);
  if (threadIdx.x != 0) return;
  const double nd = sqrt(sum);
  const float norm = (float)nd;
  const bool finite = (norm - norm) == 0.f;
  state[0] = norm;
  state[1] = finite ? (float)((double)rho / (nd + 1e-12)) : 0.f;
  state[2] = finite ? 1.f : 0.f;
  state[3] = 0.f;
  if (!finite && skipped) *skipped += 1;
}

}  // namespace mtvaf

using namespace mtvaf;

extern "C" {

// bytes of the partial-sum workspace of mtvaf_grad_sqnorm_multi over tensors of these lengths: one double per chunk.
// 0 for a bad argument (the call itself reports it).
size_t mtvaf_grad_sqnorm_workspace_bytes(int count, const long* n) {
  if (count < 0 || (count && !n)) return 0;
  long chunks = 0;
  for (int i = 0; i < count; ++i) {
    if (n[i] <= 0) return 0;
    chunks += sq_chunks(n[i]);
  }
  return (size_t)chunks * sizeof(double);
}

// Sum of squares of `count` fp32 tensors (host arrays of device pointers and lengths; any count: 48 per launch), as one double
// per chunk of 65536 elements in `partials`, tensor after tensor.
int mtvaf_grad_sqnorm_multi(int count, const float* const* g, const long* n, void* partials, size_t partials_bytes,
                            hipStream_t stream) {
  if (count < 0 || (count && (!g || !n)) || (count && !partials)) return MTVAF_ERR_ARG;
  if ((uintptr_t)partials & 7) return MTVAF_ERR_ALIGN;
  long total = 0;
  for (int i = 0; i < count; ++i) {
    if (!g[i] || n[i] <= 0) return MTVAF_ERR_ARG;
    if ((uintptr_t)g[i] & 3) return MTVAF_ERR_ALIGN;
    if (sq_chunks(n[i]) > (1L << 30)) return MTVAF_ERR_SHAPE;
    total += sq_chunks(n[i]);
  }
  if ((size_t)total * sizeof(double) > partials_bytes) return MTVAF_ERR_WORKSPACE;
  double* part = static_cast<double*>(partials);
  for (int base = 0; base < count;) {
    SqMulti t;
    long blocks = 0;
    int k = 0;
    // (a launch also ends before its grid would pass 2^30 blocks)
    for (; k < SQ_MAXT && base + k < count && blocks + sq_chunks(n[base + k]) <= (1L << 30); ++k) {
      t.g[k] = g[base + k]; t.n[k] = n[base + k];
      t.blk0[k] = (int)blocks;
      blocks += sq_chunks(n[base + k]);
    }
    t.count = k;
    t.blk0[k] = (int)blocks;
    hipLaunchKernelGGL(grad_sqnorm_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, t, part);
    MTVAF_LAUNCH_CHECK();
    part += blocks;
    base += k;
  }
  return MTVAF_OK;
}

// One block: adds `count` partials in index order (double) and writes clip_state = {norm, coef, finite, 0} (4 floats);
// max_norm <= 0: coef = 1 (report only).  A non-finite norm with skip_nonfinite != 0: coef = 0, finite = 0, *skipped += 1
// (skipped may be NULL).
int mtvaf_grad_clip_finalize(const void* partials, long count, float max_norm, int skip_nonfinite, float* clip_state,
                             int* skipped, hipStream_t stream) {
  if (count < 0 || (count && !partials) || !clip_state || max_norm != max_norm) return MTVAF_ERR_ARG;
  if (((uintptr_t)partials & 7) || ((uintptr_t)clip_state & 15) || ((uintptr_t)skipped & 3)) return MTVAF_ERR_ALIGN;
  hipLaunchKernelGGL(grad_clip_finalize_kernel, dim3(1), dim3(256), 0, stream, static_cast<const double*>(partials), count,
                     max_norm, skip_nonfinite, clip_state, skipped);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

// One block: adds `count` partials in index order (double) and writes sam_state = {norm, scale = rho / (norm + 1e-12), finite, 0}
// (4 floats, 16-byte aligned); rho finite and >= 0.  A norm that is not finite in fp32: scale = 0, finite = 0, *skipped += 1
// (skipped may be NULL).  Any bad argument: MTVAF_ERR_ARG.
int mtvaf_sam_finalize(const void* partials, long count, float rho, float* sam_state, int* skipped, hipStream_t stream) {
  if (count < 0 || (count && !partials) || !sam_state || !(rho >= 0.f) || (rho - rho) != 0.f) return MTVAF_ERR_ARG;
  if (((uintptr_t)partials & 7) || ((uintptr_t)sam_state & 15) || ((uintptr_t)skipped & 3)) return MTVAF_ERR_ARG;
  hipLaunchKernelGGL(sam_finalize_kernel, dim3(1), dim3(256), 0, stream, static_cast<const double*>(partials), count, rho, sam_state,
                     skipped);
  MTVAF_LAUNCH_CHECK();
  return MTVAF_OK;
}

}  // extern "C"
