// Host-side argument handling of the accumulating entry points and of mtvaf_layer_grads_t::accumulate, as a stand-alone program for a
// sanitizer build of the HOST code (no GPU needed: every call below is refused by the library's own checks before anything is
// launched).  Build the library's host code and this file with the same flags and run the program:
//
//   MTVAF_LIBDIR=/tmp/mtvaf_asan MTVAF_EXTRA_FLAGS="-Xarch_host -fsanitize=address,undefined" python -m mtvaf_amd.build
//   hipcc --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Iinclude tools/host_checks/accumulate_args.cpp \
//         -L/tmp/mtvaf_asan -lmtvaf_hip -Wl,-rpath,/tmp/mtvaf_asan -o /tmp/accumulate_args && /tmp/accumulate_args
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mtvaf_hip.h"

static int failures = 0;
#define EXPECT(call, want)                                                                  \
  do {                                                                                      \
    const long got_ = (long)(call);                                                         \
    if (got_ != (long)(want)) {                                                             \
      std::printf("FAIL %s:%d  %s -> %ld, expected %ld\n", __FILE__, __LINE__, #call, got_, (long)(want)); \
      ++failures;                                                                           \
    }                                                                                       \
  } while (0)

int main() {
  // the struct: `accumulate` is the last field, and a zero-initialised struct is the overwriting executor
  EXPECT(mtvaf_layer_struct_bytes(1), sizeof(mtvaf_layer_grads_t));
  EXPECT(mtvaf_layer_struct_bytes(0), sizeof(mtvaf_layer_t));
  EXPECT(offsetof(mtvaf_layer_grads_t, accumulate) + sizeof(int) <= sizeof(mtvaf_layer_grads_t), 1);
  EXPECT(offsetof(mtvaf_layer_grads_t, accumulate) > offsetof(mtvaf_layer_grads_t, dqkv_p), 1);

  // buffers that are only ever looked at as addresses (alignment checks): never dereferenced on the host
  std::vector<float> buf(1024, 0.f);
  float* const p = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(buf.data()) + 63) & ~uintptr_t(63));
  float* const odd = p + 1;  // 4-byte aligned only

  mtvaf_layer_t L;
  mtvaf_layer_grads_t G;
  std::memset(&L, 0, sizeof L);
  std::memset(&G, 0, sizeof G);
  G.accumulate = 1;
  EXPECT(mtvaf_encoder_layer_bwd(nullptr, &G, nullptr, nullptr, 0), MTVAF_ERR_ARG);
  EXPECT(mtvaf_encoder_layer_bwd(&L, nullptr, nullptr, nullptr, 0), MTVAF_ERR_ARG);
  int cu[2] = {0, 100};
  L.cu = cu; L.Mp = 100; L.Mv = 100;  // packed rows that are not whole 128-row tiles
  EXPECT(mtvaf_encoder_layer_bwd(&L, &G, nullptr, nullptr, 0), MTVAF_ERR_ARG);
  L.Mp = 128; L.Mv = 129;
  EXPECT(mtvaf_encoder_layer_bwd(&L, &G, nullptr, nullptr, 0), MTVAF_ERR_ARG);
  // plane images present but the gradient side's plane scratch missing: refused before the first launch, at accumulate 0 and 1
  L.Mv = 100; L.H = 128; L.I = 256; L.B = 1; L.S = 100; L.NH = 2;
  L.x_p = L.cx_p = L.h1_p = L.act_p = p; L.wqkv_h = L.wo_h = L.w1_h = L.w2_h = p; L.ws = p; L.ws_bytes = 64;
  for (int acc = 0; acc < 2; ++acc) {
    G.accumulate = acc;
    EXPECT(mtvaf_encoder_layer_bwd(&L, &G, nullptr, nullptr, 0), MTVAF_ERR_ARG);
  }

  // grouped pre-split launch + column-sum jobs
  const void* Ap[4] = {p, p, p, p};
  const void* Bp[4] = {p, p, p, p};
  float* C[4] = {p, p, p, p};
  int ldc[4] = {128, 128, 128, 128}, M[4] = {128, 128, 128, 128}, N[4] = {128, 128, 128, 128};
  long strides[32];
  for (int i = 0; i < 32; ++i) strides[i] = 64;
  const float* cs_src[9] = {p, p, p, p, p, p, p, p, p};
  float* cs_dst[9] = {p, p, p, p, p, p, p, p, p};
  int cs_rows[9], cs_cols[9], cs_ld[9];
  for (int j = 0; j < 9; ++j) { cs_rows[j] = 4; cs_cols[j] = 8; cs_ld[j] = 8; }
  for (int acc = 0; acc < 2; ++acc) {
    EXPECT(mtvaf_gemm_f32p_dw_group_acc(0, Ap, Bp, strides, C, ldc, M, N, 32, 0, nullptr, nullptr, nullptr, nullptr, nullptr, acc, nullptr), MTVAF_ERR_ARG);
    EXPECT(mtvaf_gemm_f32p_dw_group_acc(5, Ap, Bp, strides, C, ldc, M, N, 32, 0, nullptr, nullptr, nullptr, nullptr, nullptr, acc, nullptr), MTVAF_ERR_ARG);
    EXPECT(mtvaf_gemm_f32p_dw_group_acc(4, Ap, Bp, strides, C, ldc, M, N, 48, 0, nullptr, nullptr, nullptr, nullptr, nullptr, acc, nullptr), MTVAF_ERR_ARG);
    EXPECT(mtvaf_gemm_f32p_dw_group_acc(4, Ap, Bp, strides, C, ldc, M, N, 32, 9, cs_src, cs_rows, cs_cols, cs_ld, cs_dst, acc, nullptr), MTVAF_ERR_ARG);
    EXPECT(mtvaf_gemm_f32p_dw_group_acc(4, Ap, Bp, strides, C, ldc, M, N, 32, 2, nullptr, cs_rows, cs_cols, cs_ld, cs_dst, acc, nullptr), MTVAF_ERR_ARG);
    cs_ld[1] = 4;  // a leading dimension below the column count
    EXPECT(mtvaf_gemm_f32p_dw_group_acc(4, Ap, Bp, strides, C, ldc, M, N, 32, 2, cs_src, cs_rows, cs_cols, cs_ld, cs_dst, acc, nullptr), MTVAF_ERR_ARG);
    cs_ld[1] = 8;
    M[2] = 100;
    EXPECT(mtvaf_gemm_f32p_dw_group_acc(4, Ap, Bp, strides, C, ldc, M, N, 32, 0, nullptr, nullptr, nullptr, nullptr, nullptr, acc, nullptr), MTVAF_ERR_SHAPE);
    M[2] = 128;
    C[3] = odd;
    EXPECT(mtvaf_gemm_f32p_dw_group_acc(4, Ap, Bp, strides, C, ldc, M, N, 32, 0, nullptr, nullptr, nullptr, nullptr, nullptr, acc, nullptr), MTVAF_ERR_ALIGN);
    C[3] = p;
    strides[9] = 8;
    EXPECT(mtvaf_gemm_f32p_dw_group_acc(4, Ap, Bp, strides, C, ldc, M, N, 32, 0, nullptr, nullptr, nullptr, nullptr, nullptr, acc, nullptr), MTVAF_ERR_ALIGN);
    strides[9] = 64;
  }

  // fp32 grouped ring / split kernel group
  const float* A32[4] = {p, p, p, p};
  const float* B32[4] = {p, p, p, p};
  int lda[4] = {128, 128, 128, 128}, ldb[4] = {96, 96, 96, 96}, ldc96[4] = {96, 96, 96, 96}, N96[4] = {96, 96, 96, 96};
  float* dbias[4] = {nullptr, p, nullptr, p};
  for (int acc = 0; acc < 2; ++acc) {
    EXPECT(mtvaf_gemm_f32_dw_group_acc(5, A32, lda, B32, ldb, C, ldc96, M, N96, 64, nullptr, nullptr, dbias, p, 64, -1, acc, nullptr), MTVAF_ERR_SHAPE);
    EXPECT(mtvaf_gemm_f32_dw_group_acc(4, A32, lda, B32, ldb, C, ldc96, M, N96, 40, nullptr, nullptr, dbias, p, 64, -1, acc, nullptr), MTVAF_ERR_SHAPE);
    N96[1] = 100;
    EXPECT(mtvaf_gemm_f32_dw_group_acc(4, A32, lda, B32, ldb, C, ldc96, M, N96, 64, nullptr, nullptr, dbias, p, 64, -1, acc, nullptr), MTVAF_ERR_SHAPE);
    N96[1] = 96;
    A32[2] = odd;
    EXPECT(mtvaf_gemm_f32_dw_group_acc(4, A32, lda, B32, ldb, C, ldc96, M, N96, 64, nullptr, nullptr, dbias, p, 64, -1, acc, nullptr), MTVAF_ERR_ALIGN);
    A32[2] = p;
    // a forced split plan whose slabs do not fit the workspace: an error, never another plan
    EXPECT(mtvaf_gemm_f32_dw_group_acc(4, A32, lda, B32, ldb, C, ldc96, M, N96, 1024, nullptr, nullptr, dbias, p, 64, 4, acc, nullptr), MTVAF_ERR_WORKSPACE);
  }

  // bf16 stream-K group: shape checks come first, then the scratch that no stream has here
  const int lda8[4] = {256, 256, 256, 256}, M256[4] = {256, 256, 256, 256};
  for (int acc = 0; acc < 2; ++acc) {
    EXPECT(mtvaf_gemm_bf16x_dw_group_acc(0, Ap, lda8, Bp, lda8, C, lda8, M256, M256, 64, acc, nullptr), MTVAF_ERR_SHAPE);
    EXPECT(mtvaf_gemm_bf16x_dw_group_acc(4, Ap, lda8, Bp, lda8, C, lda8, M256, M256, 96, acc, nullptr), MTVAF_ERR_SHAPE);
    EXPECT(mtvaf_gemm_bf16x_dw_group_acc(4, Ap, lda8, Bp, lda8, C, lda8, M256, M256, 64, acc, nullptr), MTVAF_ERR_WORKSPACE);
  }
  EXPECT(mtvaf_streamk_attached(nullptr), 0);
  EXPECT(mtvaf_gemm_bf16x_dw_group_pieces(4, M256, M256, 1024, nullptr), 0);  // (no scratch on the stream)
  EXPECT(mtvaf_gemm_bf16x_dw_group_pieces(4, M256, M256, 96, nullptr), 0);

  std::printf(failures ? "accumulate_args: %d check(s) FAILED\n" : "accumulate_args: all checks passed\n", failures);
  return failures ? 1 : 0;
}
