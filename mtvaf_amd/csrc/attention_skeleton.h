// The prefix-attention kernels, ONCE: forward, the probabilities on request (the forward without V), backward query side (dQ),
// backward key side (dK, dV) and the backward dispatch, as __device__ __forceinline__ templates over an ARITHMETIC -- how a [64][64]
// tile lies in LDS and how the products over it are formed.  csrc/attention.hip (fp32 MFMA pipe), csrc/attention_f32s.hip (split bf16
// products) and csrc/attention_bf16.hip (bf16 operands, fp32 accumulation) each provide one and the thin __global__ kernels (their
// LDS, their __launch_bounds__) that call the bodies below.  Everything else -- launch geometry, the zero-fill slice of a packed
// launch, key order, masking, the log2-domain online softmax, the dropout hash, the register -> LDS double buffering with its two
// barriers, the stores -- is here and is therefore the same in all three.
//
// An arithmetic A provides (all static, __device__ __forceinline__):
//   Elem, Args                element type of Q | K | V, the context and their gradients in global memory (float / __bf16) and the
//                             argument block of its kernels (AttnArgs / ab::Args, attention_args.h, with their store_ctx / store_dqkv)
//   FWD_FETCH_AHEAD           whether the forward fetches key tile t + 1 behind the barrier that publishes tile t (the backward always
//                             does); XCD_GROUP: whether its blocks are regrouped by XCD (xcd_group)
//   Lds                       element type of its LDS tiles; RowTile / ColTile: views of one tile that is read as row fragments only /
//                             as row fragments AND columns (constructible from an Lds*)
//   stage_col()               first column of the chunk this thread stages; operand_col(g): first column a lane of group g holds
//   Stage                     staging registers of one tile: fetch_kv (rows of the [prefix ; text] key axis), fetch_rows (token rows),
//                             store(tile, stage)
//   StageDelta                rowsum(O . dO) of a staged tile in the staging layout: reduce(o, dO) -> store(del_s)
//   Operand                   the 64 values of ONE row (a lane's query or key) as the register operand of a product:
//                             load_operand(p), load_operand_dot(p, o, dot) (also adds this lane's share of rowsum(p . o))
//   rows_dot(tile, blk, x, lr, g)        [4 rows of 16-row block blk per lane group] . x over d = 64, as the MFMA result layout;
//                             rows_dot2(tile0, x0, r0, tile1, x1, r1, blk, lr, g): two of them, interleaved as the arithmetic likes it
//   FOLD                      how many 16-row blocks of probabilities / dS it gathers before it multiplies them on (1: fp32 pipe, 4, the
//                             whole tile: split and bf16)
//   cols_acc(tile, j0, p, nsub, lane, acc)   acc[dt] += tile^T(d, rows) . p over the blocks j0 .. j0 + FOLD - 1 that lie below nsub; p [FOLD]
//                             in the layout of rows_dot; cols_acc2(tile0, p0, acc0, tile1, p1, acc1, j0, nsub, lane): two of them
//   tile_without_gradient(dO, qok, Ms)   dQ side only: may report that the whole query tile has dO == 0 (see there)
//   dq_tail_exit(a)           dQ side only: whether a query tile of trailing padding writes zeros and leaves (AttnArgs::zero_tail)
//   store_delta(a, i, v)      dQ side: delta[i] = rowsum(dO . O) of a query, where the argument block has a delta
//   dq_sums(a, qtile, b, h, dq, qok, red), dkv_sums(a, ktile, b, h, dk, dv, is_text, red)   behind the stores of a block: the column sums
//                             of its dQ / of its dK | dV over text keys, where the argument block takes them; dq_sums_zero / dkv_sums_zero
//                             (a, tile, b, h): the same for a block that leaves before its loop
// The order of operations inside a product is the arithmetic's own (which blocks it folds together, plane pairs smallest first,
// MFMA operand order), and a hook that does not apply to an arithmetic is an empty inline; the bodies never ask which arithmetic
// they run.
#pragma once
#include "attention_args.h"

namespace mtvaf {

// What the two fp32 arithmetics have in common: fp32 tensors, AttnArgs, fetch-ahead and XCD grouping everywhere, delta and the
// zero_tail exit on the dQ side, no column sums.
struct F32Io {
  typedef float Elem;
  typedef AttnArgs Args;
  static constexpr bool FWD_FETCH_AHEAD = true;
  static constexpr bool XCD_GROUP = true;
  static __device__ __forceinline__ bool dq_tail_exit(const AttnArgs& a) { return a.zero_tail && !a.cu; }
  static __device__ __forceinline__ void store_delta(const AttnArgs& a, long i, float v) { a.delta[i] = v; }
  static __device__ __forceinline__ void dq_sums_zero(const AttnArgs&, int, int, int) {}
  static __device__ __forceinline__ void dq_sums(const AttnArgs&, int, int, int, const f32x4 (&)[4], bool, float*) {}
  static __device__ __forceinline__ void dkv_sums_zero(const AttnArgs&, int, int, int) {}
  static __device__ __forceinline__ void dkv_sums(const AttnArgs&, int, int, int, const f32x4 (&)[4], const f32x4 (&)[4], bool, float*) {}
};

// sources of the K and V tiles of (sentence b, head h), + the caller's column offset
template <class Args, class T>
__device__ __forceinline__ void kv_sources(const Args& a, const Sent& sn, int b, int h, int col, KvSrcT<T>& k, KvSrcT<T>& v) {
  k.pre = a.pk + ((long)b * a.P * a.NH + (long)h * a.P) * D + col;
  v.pre = a.pv + ((long)b * a.P * a.NH + (long)h * a.P) * D + col;
  k.txt = a.qkv + sn.tok0 * 3 * a.H + a.H + h * D + col;
  v.txt = k.txt + a.H;
}

// ---------------------------------------------------------------------------------------------
// forward: grid (ceil(S/64), NH, B [+ 1]), 256 threads; wave w owns queries q0 + 16 w .. + 15
// Ms [KT]: additive mask * log2(e) of the tile's keys (-1e30 beyond T)
// ---------------------------------------------------------------------------------------------
template <class A, bool PM = false>
__device__ __forceinline__ void attn_fwd_body(const typename A::Args& a, typename A::RowTile Ks, typename A::ColTile Vs, float* Ms,
                                              int* t_eff_slot, const float* pmask = nullptr) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lq = lane & 15, g = lane >> 4;
  int bx = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  if constexpr (A::XCD_GROUP) xcd_group(gridDim.x, gridDim.y, a.B, bx, h, b);
  const int q = bx * 64 + wave * 16 + lq;
  if (a.cu && b == a.B) {  // (block-uniform) the rows that pad the packed image: zeros (0 x NaN of an unwritten row would poison dW)
    const int r0 = a.cu[a.B];
    for (int r = bx * 16 + (threadIdx.x >> 4); r < a.pad_rows; r += gridDim.x * 16)
      store_ctx(a, (long)(r0 + r), h * D + (threadIdx.x & 15) * 4, f32x4{0.f, 0.f, 0.f, 0.f});
    return;
  }
  b = slot_sentence(a, b);
  const Sent sn = sentence(a, b);
  const int Sb = sn.n;
  if (bx * 64 >= Sb) return;  // (block-uniform; packed rows: a query tile beyond the sentence)
  const int Tf = a.P + a.S;   // row length of the additive mask
  const int T = a.cu ? a.P + Sb : effective_keys(a.addmask + (long)b * Tf, a.P, a.S, t_eff_slot);  // trailing padding keys are skipped
  const bool qok = q < Sb;
  // The last query tile of a sentence is rarely full (74 tokens: queries 64 .. 73 live in wave 0 of the second tile); a wave whose 16
  // queries all lie beyond the sentence would run every product and exponential of the key loop for rows nobody stores -- on the
  // matrix pipe it shares with the live waves of the other blocks on its SIMD.  It skips the arithmetic (same results: bit-identical).
  const bool wave_live = __builtin_amdgcn_readfirstlane(q - lq) < Sb;
  const float inv_keep = a.p_drop > 0.f ? 1.f / (1.f - a.p_drop) : 1.f;
  const uint32_t rowh = attn_dropout_rowhash(attn_epoch_key(a.drop_key, a.epoch), (uint32_t)((b * a.NH + h) * a.S + q));
  const float sc2 = a.scale * LOG2E;  // scores are kept in the log2 domain: one v_exp_f32 per probability

  KvSrcT<typename A::Elem> ksrc, vsrc;
  kv_sources(a, sn, b, h, A::stage_col(), ksrc, vsrc);
  const int ldt = 3 * a.H;

  const typename A::Operand qf = A::load_operand(a.qkv + (sn.tok0 + min(q, Sb - 1)) * 3 * a.H + h * D + A::operand_col(g));
  f32x4 oacc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) oacc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = NEG_BIG, l_run = 0.f;

  // The next key tile travels global -> registers while the current one is being multiplied: its loads are issued
  // right behind the barrier that publishes the current tile and are first needed at the top of the next iteration
  // (A::FWD_FETCH_AHEAD; an arithmetic without it loads a tile at the top of its own iteration).
  typename A::Stage kst, vst;
  float mreg = NEG_BIG;
  auto fetch = [&](int t0) {
    A::fetch_kv(kst, ksrc, a.P, T, ldt, t0);
    A::fetch_kv(vst, vsrc, a.P, T, ldt, t0);
    if (threadIdx.x < KT) mreg = mask_at<PM>(a, b, Tf, min(t0 + (int)threadIdx.x, T - 1), pmask);
  };
  if constexpr (A::FWD_FETCH_AHEAD) fetch(0);
  for (int t0 = 0; t0 < T; t0 += KT) {
    if constexpr (!A::FWD_FETCH_AHEAD) fetch(t0);
    __syncthreads();
    A::store(Ks, kst);
    A::store(Vs, vst);
    if (threadIdx.x < KT) Ms[threadIdx.x] = (t0 + (int)threadIdx.x < T) ? mreg * LOG2E : NEG_BIG;
    __syncthreads();
    if constexpr (A::FWD_FETCH_AHEAD) {
      if (t0 + KT < T) fetch(t0 + KT);
    }
    if (!wave_live) continue;  // (wave-uniform) no live query in this wave: it only stages and synchronises
    const int nsub = min(4, (T - t0 + 15) >> 4);  // 16-key blocks of this tile that hold real keys
    f32x4 s[4];
    float tmax = NEG_BIG;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s[j] = f32x4{NEG_BIG, NEG_BIG, NEG_BIG, NEG_BIG};
      if (j < nsub) {
        const f32x4 acc = A::rows_dot(Ks, j, qf, lq, g);
        const f32x4 mv = *reinterpret_cast<const f32x4*>(Ms + 16 * j + 4 * g);
        s[j] = acc * sc2 + mv;
        tmax = fmaxf(tmax, fmaxf(fmaxf(s[j].x, s[j].y), fmaxf(s[j].z, s[j].w)));
      }
    }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
    const float m_new = fmaxf(m_run, tmax);
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
    float psum = 0.f;
    const uint32_t cterm0 = (uint32_t)(t0 + 4 * g) * ATTN_DROP_C2;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = __builtin_amdgcn_exp2f(s[j][r] - m_new);
        psum += p;
        float pd = p;
        if (a.p_drop > 0.f)
          pd = attn_dropout_keep2(rowh, cterm0 + (uint32_t)(16 * j + r) * ATTN_DROP_C2, a.drop_thr) ? p * inv_keep : 0.f;
        s[j][r] = pd;
      }
    psum += __shfl_xor(psum, 16, 64);
    psum += __shfl_xor(psum, 32, 64);
    l_run = l_run * alpha + psum;
    m_run = m_new;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) oacc[dt] *= alpha;
#pragma unroll
    for (int j0 = 0; j0 < 4; j0 += A::FOLD) A::cols_acc(Vs, j0, s + j0, nsub, lane, oacc);  // O^T[d][q] += V^T[d][key] Pd^T[key][q]
  }
  if (qok) {
    const float inv_l = 1.f / l_run;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) store_ctx(a, sn.tok0 + q, h * D + 16 * dt + 4 * g, oacc[dt] * inv_l);
    if (g == 0) a.lse[((long)b * a.NH + h) * a.S + q] = (m_run + log2f(l_run)) * LN2;
  }
}

// ---------------------------------------------------------------------------------------------
// attention probabilities on request (output_attentions): the forward without V.  probs [B, NH, S, P + S] dense fp32, EVERY element
// written; mass [B, NH, S] = sum of a row over the prefix slots.  Same grid, staging, key order, masking and log2-domain scores as
// the forward (padded layout only).  TWO passes over the key tiles of a 64-query tile: the first keeps the running (max, sum), the
// second recomputes the scores and stores exp2(s - m) / l -- no [64][T] score tile is parked in LDS.  A score block has a query on a
// lane (consecutive lanes = consecutive ROWS of the output); each wave turns its [16 queries][64 keys] block through its own
// [16][LDP] slice of Ps so that a store instruction writes 64 consecutive keys of one row (4-byte stores: T is not a multiple of 4).
// ---------------------------------------------------------------------------------------------
constexpr int LDP = 68;  // row stride (floats) of the transposing buffer: 16-byte aligned rows for the b128 writes

template <class A>
__device__ __forceinline__ void attn_probs_body(const typename A::Args& a, const ProbsOut& o, typename A::RowTile Ks, float* Ps, float* Ms,
                                                int* t_eff_slot) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lq = lane & 15, g = lane >> 4;
  int bx = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  if constexpr (A::XCD_GROUP) xcd_group(gridDim.x, gridDim.y, a.B, bx, h, b);
  const Sent sn = sentence(a, b);
  const int S = a.S, Tf = a.P + a.S;
  // keys behind the last unmasked text position: exact zeros in the reference too (exp(-10000 - max) underflows), stored below
  const int T = effective_keys(a.addmask + (long)b * Tf, a.P, S, t_eff_slot);
  const int qw = bx * 64 + wave * 16;  // first query of this wave
  const int q = qw + lq;
  const bool wave_live = qw < S;
  const float sc2 = a.scale * LOG2E;
  const bool zrow = o.zero_masked_queries && a.addmask[(long)b * Tf + a.P + min(q, S - 1)] <= -5000.f;

  KvSrcT<typename A::Elem> ksrc, vsrc;
  kv_sources(a, sn, b, h, A::stage_col(), ksrc, vsrc);
  const int ldt = 3 * a.H;
  const typename A::Operand qf = A::load_operand(a.qkv + (sn.tok0 + min(q, S - 1)) * 3 * a.H + h * D + A::operand_col(g));

  // one sweep over the key tiles [0, Tend): stage (next tile in flight as in the forward), scores of the live waves -> tile(t0, s)
  auto sweep = [&](int Tend, auto&& tile) {
    typename A::Stage kst;
    float mreg = NEG_BIG;
    auto fetch = [&](int t0) {
      A::fetch_kv(kst, ksrc, a.P, T, ldt, t0);
      if (threadIdx.x < KT) mreg = mask_at(a, b, Tf, min(t0 + (int)threadIdx.x, T - 1));
    };
    if (Tend > 0) fetch(0);
    for (int t0 = 0; t0 < Tend; t0 += KT) {
      __syncthreads();
      A::store(Ks, kst);
      if (threadIdx.x < KT) Ms[threadIdx.x] = (t0 + (int)threadIdx.x < T) ? mreg * LOG2E : NEG_BIG;
      __syncthreads();
      if (t0 + KT < Tend) fetch(t0 + KT);
      if (!wave_live) continue;  // (wave-uniform) no query of this wave exists: it only stages and synchronises
      const int nsub = min(4, (T - t0 + 15) >> 4);
      f32x4 s[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        s[j] = f32x4{NEG_BIG, NEG_BIG, NEG_BIG, NEG_BIG};
        if (j < nsub) {
          const f32x4 acc = A::rows_dot(Ks, j, qf, lq, g);
          const f32x4 mv = *reinterpret_cast<const f32x4*>(Ms + 16 * j + 4 * g);
          s[j] = acc * sc2 + mv;
        }
      }
      tile(t0, s);
    }
  };

  float m_run = NEG_BIG, l_run = 0.f;
  sweep(T, [&](int, f32x4(&s)[4]) {
    float tmax = NEG_BIG;
#pragma unroll
    for (int j = 0; j < 4; ++j) tmax = fmaxf(tmax, fmaxf(fmaxf(s[j].x, s[j].y), fmaxf(s[j].z, s[j].w)));
    tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
    const float m_new = fmaxf(m_run, tmax);
    float psum = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) psum += __builtin_amdgcn_exp2f(s[j][r] - m_new);
    psum += __shfl_xor(psum, 16, 64);
    psum += __shfl_xor(psum, 32, 64);
    l_run = l_run * __builtin_amdgcn_exp2f(m_run - m_new) + psum;
    m_run = m_new;
  });

  const float inv_l = zrow ? 0.f : 1.f / l_run;  // (every probability is finite: 0 * p = 0 exactly)
  const long row0 = ((long)b * a.NH + h) * S;    // first row of this (sentence, head) in probs / mass
  float* Pw = Ps + wave * 16 * LDP;
  float pmass = 0.f;
  sweep(o.probs ? T : a.P, [&](int t0, f32x4(&s)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[j][r] = __builtin_amdgcn_exp2f(s[j][r] - m_run) * inv_l;  // keys beyond T: exp2(-1e30 - m) = 0
        pmass += (t0 + 16 * j + 4 * g + r < a.P) ? s[j][r] : 0.f;
      }
    }
    if (!o.probs) return;
#pragma unroll
    for (int j = 0; j < 4; ++j) *reinterpret_cast<f32x4*>(Pw + lq * LDP + 16 * j + 4 * g) = s[j];
    // one wave: LDS operations execute in program order, the fences only keep the compiler from moving the reads above the writes
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (t0 + lane < Tf) {
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (qw + i < S) o.probs[(row0 + qw + i) * Tf + t0 + lane] = Pw[i * LDP + lane];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();  // (the next tile overwrites the slice)
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  });
  if (!wave_live) return;
  if (o.probs) {  // whole key tiles of trailing padding
    for (int t = ((T + KT - 1) / KT) * KT + lane; t < Tf; t += KT)
      for (int i = 0; i < 16 && qw + i < S; ++i) o.probs[(row0 + qw + i) * Tf + t] = 0.f;
  }
  if (o.mass) {
    pmass += __shfl_xor(pmass, 16, 64);
    pmass += __shfl_xor(pmass, 32, 64);
    if (g == 0 && q < S) o.mass[row0 + q] = pmass;
  }
}

// ---------------------------------------------------------------------------------------------
// backward, query side: dQ for 64 queries per block; loop over key tiles as in the forward.  What leaves the block beside dQ is the
// arithmetic's (its output hooks: delta = rowsum(dO.O), or the column sums of dQ through red)
// ---------------------------------------------------------------------------------------------
template <class A, bool PM = false>
__device__ __forceinline__ void attn_bwd_dq_body(const typename A::Args& a, int qtile, int b, int h, typename A::ColTile Ks,
                                                 typename A::RowTile Vs, float* Ms, float* red, int* t_eff_slot,
                                                 const float* pmask = nullptr) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lq = lane & 15, g = lane >> 4;
  const int q = qtile * 64 + wave * 16 + lq;
  const Sent sn = sentence(a, b);
  const int Sb = sn.n;
  if (qtile * 64 >= Sb) {  // (block-uniform) a query tile beyond the sentence
    A::dq_sums_zero(a, qtile, b, h);
    return;
  }
  const int Tf = a.P + a.S;
  const int T = a.cu ? a.P + Sb : effective_keys(a.addmask + (long)b * Tf, a.P, a.S, t_eff_slot);
  const bool qok = q < Sb;
  const bool wave_live = __builtin_amdgcn_readfirstlane(q - lq) < Sb;
  if (A::dq_tail_exit(a) && qtile * 64 >= T - a.P) {  // (block-uniform) a tile of trailing padding: dQ = 0, nothing to read
    if (qok) {
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) store_dqkv(a, sn.tok0 + q, h * D + 16 * dt + 4 * g, z);
      if (g == 0) A::store_delta(a, ((long)b * a.NH + h) * a.S + q, 0.f);
    }
    return;
  }
  const float inv_keep = a.p_drop > 0.f ? 1.f / (1.f - a.p_drop) : 1.f;
  const uint32_t rowh = attn_dropout_rowhash(attn_epoch_key(a.drop_key, a.epoch), (uint32_t)((b * a.NH + h) * a.S + q));
  const float sc2 = a.scale * LOG2E;

  KvSrcT<typename A::Elem> ksrc, vsrc;
  kv_sources(a, sn, b, h, A::stage_col(), ksrc, vsrc);
  const int ldt = 3 * a.H;

  float dl = 0.f;
  const long qrow = sn.tok0 + min(q, Sb - 1);
  const int ocol = h * D + A::operand_col(g);
  const typename A::Operand qf = A::load_operand(a.qkv + qrow * 3 * a.H + ocol);
  const typename A::Operand dof = A::load_operand_dot(a.dctx + qrow * a.H + ocol, a.ctx + qrow * a.H + ocol, dl);
  dl += __shfl_xor(dl, 16, 64);
  dl += __shfl_xor(dl, 32, 64);
  // rows beyond S: lse = +1e30 makes every probability (and with it ds) exactly 0
  const float lse2 = qok ? a.lse[((long)b * a.NH + h) * a.S + q] * LOG2E : 1.0e30f;
  if (qok && g == 0) A::store_delta(a, ((long)b * a.NH + h) * a.S + q, dl);

  f32x4 dq[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) dq[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (A::tile_without_gradient(dof, qok, Ms)) {  // dS = 0 and dQ = 0 exactly: write the zeros and skip the key loop
    if (qok) {
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) store_dqkv(a, sn.tok0 + q, h * D + 16 * dt + 4 * g, dq[dt]);
    }
    return;
  }

  typename A::Stage kst, vst;  // (the next key tile is fetched while the current one is multiplied, as in the forward)
  float mreg = NEG_BIG;
  auto fetch = [&](int t0) {
    A::fetch_kv(kst, ksrc, a.P, T, ldt, t0);
    A::fetch_kv(vst, vsrc, a.P, T, ldt, t0);
    if (threadIdx.x < KT) mreg = mask_at<PM>(a, b, Tf, min(t0 + (int)threadIdx.x, T - 1), pmask);
  };
  fetch(0);
  for (int t0 = 0; t0 < T; t0 += KT) {
    __syncthreads();
    A::store(Ks, kst);
    A::store(Vs, vst);
    if (threadIdx.x < KT) Ms[threadIdx.x] = (t0 + (int)threadIdx.x < T) ? mreg * LOG2E : NEG_BIG;
    __syncthreads();
    if (t0 + KT < T) fetch(t0 + KT);
    if (!wave_live) continue;  // (wave-uniform; as in the forward.  dq stays zero: dq_sums reads it through qok)
    const int nsub = min(4, (T - t0 + 15) >> 4);
    const uint32_t cterm0 = (uint32_t)(t0 + 4 * g) * ATTN_DROP_C2;
#pragma unroll
    for (int j0 = 0; j0 < 4; j0 += A::FOLD) {
      f32x4 ds[A::FOLD];
#pragma unroll
      for (int jj = 0; jj < A::FOLD; ++jj) {
        const int j = j0 + jj;
        ds[jj] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (j < nsub) {
          f32x4 s, dp;
          A::rows_dot2(Ks, qf, s, Vs, dof, dp, j, lq, g);
          const f32x4 mv = *reinterpret_cast<const f32x4*>(Ms + 16 * j + 4 * g);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float p = __builtin_amdgcn_exp2f(s[r] * sc2 + mv[r] - lse2);
            float dpe = dp[r];
            if (a.p_drop > 0.f)
              dpe = attn_dropout_keep2(rowh, cterm0 + (uint32_t)(16 * j + r) * ATTN_DROP_C2, a.drop_thr) ? dpe * inv_keep : 0.f;
            ds[jj][r] = p * (dpe - dl) * a.scale;
          }
        }
      }
      A::cols_acc(Ks, j0, ds, nsub, lane, dq);  // dQ^T[d][q] += K^T[d][key] dS^T[key][q]
    }
  }
  if (qok) {
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) store_dqkv(a, sn.tok0 + q, h * D + 16 * dt + 4 * g, dq[dt]);
  }
  A::dq_sums(a, qtile, b, h, dq, qok, red);
}

// ---------------------------------------------------------------------------------------------
// backward, key side: dK, dV for 64 keys of the [prefix ; text] axis per block (prefix slots write dpk / dpv -- the gradient that
// flows on to the prompt generator); loop over query tiles.
// lse_s [KT] = lse * log2(e) (+1e30 for rows beyond S); del_s [KT] = rowsum(dO.O), computed here from the staged dO tile and the
// matching O rows so that this side does not depend on the query side (both run in one launch); rh_s [KT] = dropout row hashes of
// the tile's queries.  Output hook: the column sums of dK | dV over the block's text keys (through red).
// ---------------------------------------------------------------------------------------------
template <class A, bool PM = false>
__device__ __forceinline__ void attn_bwd_dkv_body(const typename A::Args& a, int ktile, int b, int h, typename A::ColTile Qs,
                                                  typename A::ColTile dOs, float* lse_s, float* del_s, uint32_t* rh_s, float* red,
                                                  int* t_eff_slot, const float* pmask = nullptr) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lk = lane & 15, g = lane >> 4;
  const Sent sn = sentence(a, b);
  const int Sb = sn.n;
  const int T = a.cu ? a.P + Sb : effective_keys(a.addmask + (long)b * (a.P + a.S), a.P, a.S, t_eff_slot);  // keys >= T: trailing padding
  const int Tf = a.cu ? T : a.P + a.S;  // (packed rows: keys beyond the sentence do not exist)
  const int key = ktile * 64 + wave * 16 + lk;
  if (ktile * 64 >= T) {  // (block-uniform) a key tile of trailing padding only: exact zeros, no query loop
    if (key < Tf) {
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        store_dqkv(a, sn.tok0 + (key - a.P), a.H + h * D + 16 * dt + 4 * g, z);
        store_dqkv(a, sn.tok0 + (key - a.P), 2 * a.H + h * D + 16 * dt + 4 * g, z);
      }
    }
    A::dkv_sums_zero(a, ktile, b, h);
    return;
  }
  const bool kok = key < T;
  const bool wave_live = (int)(ktile * 64 + wave * 16) < T;
  const int keyc = min(key, T - 1);
  const float inv_keep = a.p_drop > 0.f ? 1.f / (1.f - a.p_drop) : 1.f;
  const float mval2 = kok ? mask_at<PM>(a, b, Tf, key, pmask) * LOG2E : NEG_BIG;  // keys beyond T: probability exactly 0
  const float sc2 = a.scale * LOG2E;
  const uint32_t cterm = (uint32_t)key * ATTN_DROP_C2;

  KvSrcT<typename A::Elem> ksrc, vsrc;
  kv_sources(a, sn, b, h, A::operand_col(g), ksrc, vsrc);
  const typename A::Operand kf = A::load_operand(kv_row_ptr(ksrc, keyc, a.P, 3 * a.H));
  const typename A::Operand vf = A::load_operand(kv_row_ptr(vsrc, keyc, a.P, 3 * a.H));
  f32x4 dk[4], dv[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) dk[i] = dv[i] = f32x4{0.f, 0.f, 0.f, 0.f};

  const typename A::Elem* qsrc = a.qkv + sn.tok0 * 3 * a.H + h * D + A::stage_col();
  const typename A::Elem* dosrc = a.dctx + sn.tok0 * a.H + h * D + A::stage_col();
  const typename A::Elem* osrc = a.ctx + sn.tok0 * a.H + h * D + A::stage_col();
  const uint32_t row_base = (uint32_t)((b * a.NH + h) * a.S);

  // the next query tile (Q, dO, O rows, lse) is fetched while the current one is multiplied
  typename A::Stage qst, dst, ost;
  float lreg = 1.0e30f;
  auto fetch = [&](int q0) {
    A::fetch_rows(qst, dst, ost, qsrc, dosrc, osrc, a.H, q0, Sb);
    if (threadIdx.x < KT) lreg = a.lse[((long)b * a.NH + h) * a.S + min(q0 + (int)threadIdx.x, Sb - 1)] * LOG2E;
  };
  // (zero_tail: queries from the last unmasked position on have dO = 0 exactly -- no contribution, see AttnArgs)
  const int Sq = (a.zero_tail && !a.cu) ? min(Sb, T - a.P) : Sb;
  if (Sq > 0) fetch(0);
  for (int q0 = 0; q0 < Sq; q0 += KT) {
    typename A::StageDelta dsum;
    dsum.reduce(ost, dst);
    const float lcur = lreg;
    __syncthreads();
    A::store(Qs, qst);
    A::store(dOs, dst);
    dsum.store(del_s);
    if (threadIdx.x < KT) {
      const int qq = q0 + threadIdx.x;
      lse_s[threadIdx.x] = qq < Sb ? lcur : 1.0e30f;
      rh_s[threadIdx.x] = attn_dropout_rowhash(attn_epoch_key(a.drop_key, a.epoch), row_base + (uint32_t)qq);
    }
    __syncthreads();
    if (q0 + KT < Sq) fetch(q0 + KT);
    // a wave whose 16 keys all lie beyond T (last key tile) only takes part in the staging and the barriers
    const int nsub = wave_live ? min(4, (Sq - q0 + 15) >> 4) : 0;
#pragma unroll
    for (int i0 = 0; i0 < 4; i0 += A::FOLD) {
      f32x4 pd[A::FOLD], ds[A::FOLD];
#pragma unroll
      for (int ii = 0; ii < A::FOLD; ++ii) {
        const int i = i0 + ii;
        pd[ii] = ds[ii] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (i < nsub) {
          f32x4 s, dp;  // S[q][key] and dP[q][key]: lane = key, rows q = 16 i + 4 g + r
          A::rows_dot2(Qs, kf, s, dOs, vf, dp, i, lk, g);
          const f32x4 lse4 = *reinterpret_cast<const f32x4*>(lse_s + 16 * i + 4 * g);
          const f32x4 del4 = *reinterpret_cast<const f32x4*>(del_s + 16 * i + 4 * g);
          const uint4 rh4 = *reinterpret_cast<const uint4*>(rh_s + 16 * i + 4 * g);
          const uint32_t rh[4] = {rh4.x, rh4.y, rh4.z, rh4.w};
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float p = __builtin_amdgcn_exp2f(s[r] * sc2 + mval2 - lse4[r]);
            float dpe = dp[r], pdr = p;
            if (a.p_drop > 0.f) {
              const bool keep = attn_dropout_keep2(rh[r], cterm, a.drop_thr);
              pdr = keep ? p * inv_keep : 0.f;
              dpe = keep ? dpe * inv_keep : 0.f;
            }
            pd[ii][r] = pdr;
            ds[ii][r] = p * (dpe - del4[r]) * a.scale;
          }
        }
      }
      // dV^T[d][key] += dO^T[d][q] Pd[q][key];  dK^T[d][key] += Q^T[d][q] dS[q][key]
      A::cols_acc2(dOs, pd, dv, Qs, ds, dk, i0, nsub, lane);
    }
  }
  if (!kok && key < Tf) {  // trailing padding inside a partially valid tile
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      store_dqkv(a, sn.tok0 + (key - a.P), a.H + h * D + 16 * dt + 4 * g, z);
      store_dqkv(a, sn.tok0 + (key - a.P), 2 * a.H + h * D + 16 * dt + 4 * g, z);
    }
  }
  if (kok) {
    if (key < a.P) {
      float* dkrow = a.dpk + ((long)b * a.P * a.NH + (long)h * a.P + key) * D;
      float* dvrow = a.dpv + ((long)b * a.P * a.NH + (long)h * a.P + key) * D;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        *reinterpret_cast<f32x4*>(dkrow + 16 * dt + 4 * g) = dk[dt];
        *reinterpret_cast<f32x4*>(dvrow + 16 * dt + 4 * g) = dv[dt];
      }
    } else {
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        store_dqkv(a, sn.tok0 + (key - a.P), a.H + h * D + 16 * dt + 4 * g, dk[dt]);
        store_dqkv(a, sn.tok0 + (key - a.P), 2 * a.H + h * D + 16 * dt + 4 * g, dv[dt]);
      }
    }
  }
  A::dkv_sums(a, ktile, b, h, dk, dv, kok && key >= a.P, red);
}

// One launch for the whole attention backward: blocks [0, nq) of x are query tiles (dQ), the rest key tiles (dK, dV).  The two
// sides are independent (the key side recomputes delta), so they share the machine and need neither atomics nor a second stream.
// tile0, tile1: two LDS tiles of the arithmetic; small [3 KT] floats; red: what the arithmetic's column-sum hooks reduce through
// ([8 * 64] floats, or NULL where they are empty).
template <class A, bool PM = false>
__device__ __forceinline__ void attn_bwd_body(const typename A::Args& a, int nq, typename A::Lds* tile0, typename A::Lds* tile1,
                                              float* small, float* red, int* t_eff_slot, const float* pmask = nullptr) {
  if (a.cu && (int)blockIdx.z == a.B) {  // (block-uniform) zero dQ | dK | dV of the rows that pad the packed image
    const int r0 = a.cu[a.B], h = blockIdx.y;
    for (int r = blockIdx.x * 16 + (threadIdx.x >> 4); r < a.pad_rows; r += gridDim.x * 16)
#pragma unroll
      for (int c = 0; c < 3; ++c)
        store_dqkv(a, (long)(r0 + r), c * a.H + h * D + (threadIdx.x & 15) * 4, f32x4{0.f, 0.f, 0.f, 0.f});
    return;
  }
  int bx = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  if constexpr (A::XCD_GROUP) xcd_group(gridDim.x, gridDim.y, a.B, bx, h, b);
  b = slot_sentence(a, b);
  if (bx < nq) {
    attn_bwd_dq_body<A, PM>(a, bx, b, h, typename A::ColTile{tile0}, typename A::RowTile{tile1}, small, red, t_eff_slot, pmask);
  } else {
    attn_bwd_dkv_body<A, PM>(a, bx - nq, b, h, typename A::ColTile{tile0}, typename A::ColTile{tile1}, small, small + KT,
                             reinterpret_cast<uint32_t*>(small + 2 * KT), red, t_eff_slot, pmask);
  }
}

}  // namespace mtvaf
