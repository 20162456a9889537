/* mtvaf_hip.h -- C ABI of libmtvaf_hip.so: the MI355X (gfx950) kernels behind MTVAF's prefix-fused
 * BERT/RoBERTa forward/backward path.
 *
 * The reference (MKMaS-GUET/MTVAF) has no FFI layer: the path sits behind Python nn.Modules
 * (models/bert_model.py::TVNetSAModel2, models/modeling_bert.py::BertModel).  Each entry point below
 * replaces the eager torch ops of the cited reference lines; the Python side (mtvaf_amd/hip.py) binds
 * them with ctypes and wraps them in torch.autograd.Functions inside modules that keep the reference's
 * class names, constructor/forward signatures and parameter names.
 *
 * Conventions
 *   - all tensors are dense row-major fp32 device buffers owned by the caller (torch); the library never
 *     allocates; scratch is passed in (`*_workspace_bytes` queries give the size);
 *   - every call only enqueues work on `stream` (a hipStream_t) and never synchronises;
 *   - return 0 on success, <0 = MTVAF_ERR_* (bad shape / alignment / argument / workspace), >0 = hipError_t;
 *   - float4 vector access: row strides are multiples of 4 floats and bases 16-byte aligned unless a
 *     function says otherwise (the GEMM falls back to scalar loads when they are not);
 *   - dropout masks are a pure function of (seed, offset, element index): backward calls take the same
 *     (p_drop, seed, offset) as their forward and regenerate the mask;
 *   - `accumulate` != 0 adds parameter gradients into the destination instead of overwriting it.
 */
#ifndef MTVAF_HIP_H
#define MTVAF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* hipStream_t, spelled as hip_runtime_api.h spells it: the struct stays incomplete, so this header needs no HIP header and is
 * valid C99, and the library's own sources -- every one includes this header -- define the entry points with hipStream_t
 * against these very prototypes.  A plain pointer in the ABI (ctypes: c_void_p). */
typedef struct ihipStream_t* mtvaf_stream_t;

#define MTVAF_OK 0
#define MTVAF_ERR_SHAPE (-1)
#define MTVAF_ERR_ALIGN (-2)
#define MTVAF_ERR_ARG (-3)
#define MTVAF_ERR_WORKSPACE (-4)

/* operand layouts of mtvaf_gemm_f32: KC = reduction index contiguous, KM = reduction index is the row */
#define MTVAF_KC 0
#define MTVAF_KM 1
/* epilogues */
#define MTVAF_EPI_NONE 0
#define MTVAF_EPI_GELU 1  /* C = gelu_erf(acc + bias), pre-activation -> aux  (modeling_bert.py:420-421) */
#define MTVAF_EPI_TANH 2  /* C = tanh(acc + bias)                            (bert_model.py:446-454)   */
#define MTVAF_EPI_DGELU 3 /* C = acc * gelu_erf'(aux)                                                   */
#define MTVAF_EPI_DTANH 4 /* C = acc * (1 - aux^2)                                                      */

/* Device-side dropout epoch for captured launches (HIP graph replay freezes kernel arguments, so host-fed (seed, offset)
 * pairs would repeat the same masks): while a device uint64 word is registered, every dropout-drawing kernel of the
 * library folds its value into its counter stream; mtvaf_rng_epoch_advance (*word += 1, captured as the first node of a
 * training-step graph) makes every replay draw fresh masks, identically in its forward and backward kernels.  NULL
 * restores host-fed masks.  Process-global state (like the launch profiler). */
int mtvaf_rng_set_epoch_ptr(const uint64_t* dev_word);
int mtvaf_rng_epoch_advance(uint64_t* dev_word, mtvaf_stream_t stream);
int mtvaf_version(void);
int mtvaf_device_cus(void);

/* ---- dense projections (fp32 MFMA): nn.Linear forward / dX / dW ------------------------------------
 * replaces query/key/value (modeling_bert.py:266,283-284), BertSelfOutput.dense (:353),
 * BertIntermediate.dense + GELU (:420-421), BertOutput.dense (:433), encoder_conv / projectors /
 * img_classifier (bert_model.py:446-459, 541-542, 552, 568), fc (bert_model.py:510) and their autograd
 * backward.  C[M,N] = opA[M,K] . opB[K,N] (+bias[N]) with epilogue `epi`; cfg/splits < 0 = heuristic.
 * allow_split enables a deterministic split-K (ordered slab reduction) through `workspace`. */
size_t mtvaf_gemm_f32_workspace_bytes(int M, int N, int K, int allow_split);
/* launch profiler (bench.py roofline): HIP events around the main GEMM kernel of every call, on its stream */
int mtvaf_prof_start(int capacity);
int mtvaf_prof_stop(int* n_out, int* keys /* [n][8] */, float* ms /* [n] */, int max_records);
int mtvaf_gemm_f32_plan(int layout_a, int layout_b, int M, int N, int K, int epi, int allow_split, int* cfg,
                        int* splits);
int mtvaf_gemm_f32(int layout_a, int layout_b, const float* A, int lda, const float* B, int ldb, float* C, int ldc,
                   int M, int N, int K, const float* bias, int epi, float* aux, int ldaux, int accumulate,
                   int allow_split, void* workspace, size_t workspace_bytes, int cfg, int splits,
                   mtvaf_stream_t stream);

/* bf16-compute variant for the mixed-precision configurations: identical contract (fp32 buffers), operands are
 * rounded to bf16 while staged and multiplied on the bf16 MFMA with fp32 accumulation. */
int mtvaf_gemm_bf16(int layout_a, int layout_b, const float* A, int lda, const float* B, int ldb, float* C, int ldc,
                    int M, int N, int K, const float* bias, int epi, float* aux, int ldaux, int accumulate,
                    int allow_split, void* workspace, size_t workspace_bytes, int cfg, int splits,
                    mtvaf_stream_t stream);

/* ---- fused prefix self-attention ---------------------------------------------------------------------
 * replaces BertSelfAttention.forward's prefix concat + scores + mask + softmax + dropout + PV + head merge
 * (modeling_bert.py:282-286, 303, 320-337; modeling_roberta.py:218-222) and its backward.
 * qkv [B*S,3H] token-major (Q|K|V); pk/pv [B,P*H] raw reshape(bsz,12,-1,64) slabs (bert_model.py:585);
 * addmask [B,P+S] = (1-mask)*-10000; ctx [B*S,H]; lse [B,NH,S].  head_dim must be 64. */
int mtvaf_prefix_attn_fwd(const float* qkv, const float* pk, const float* pv, const float* addmask, float* ctx,
                          float* lse, int B, int S, int P, int NH, int head_dim, float p_drop, uint64_t seed,
                          uint64_t offset, mtvaf_stream_t stream);
int mtvaf_prefix_attn_bwd(const float* dctx, const float* qkv, const float* pk, const float* pv,
                          const float* addmask, const float* ctx, const float* lse, float* delta, float* dqkv,
                          float* dpk, float* dpv, int B, int S, int P, int NH, int head_dim, float p_drop,
                          uint64_t seed, uint64_t offset, mtvaf_stream_t stream);
/* mtvaf_prefix_attn_bwd for callers that vouch (zero_tail != 0) that dctx is EXACTLY zero for the queries behind a sentence's
 * last unmasked text position -- trailing padding nothing downstream reads: the contract under which the weight gradients
 * walk k-tile lists.  Those queries have dQ = 0 and add nothing to dK / dV, so the query loops stop there; under the
 * contract the results equal mtvaf_prefix_attn_bwd's bit for bit. */
int mtvaf_prefix_attn_bwd_tail(const float* dctx, const float* qkv, const float* pk, const float* pv, const float* addmask,
                               const float* ctx, const float* lse, float* delta, float* dqkv, float* dpk, float* dpv, int B,
                               int S, int P, int NH, int head_dim, float p_drop, uint64_t seed, uint64_t offset, int zero_tail,
                               mtvaf_stream_t stream);

/* The attention probabilities on request (output_attentions; modeling_bert.py:325, 339): the forward without V, by the same
 * arithmetic (mtvaf_f32_split).  probs [B,NH,S,P+S] dense fp32 = softmax_t(Q.[Kp;K]^T / 8 + addmask), before dropout; EVERY element
 * is written (no memset needed), keys behind a sentence's last unmasked text position as exactly 0.  prefix_mass [B,NH,S] (may be
 * NULL) = sum_{t<P} probs[b,h,q,t], the share of a token's attention that goes to the visual slots.  zero_masked_queries != 0: the
 * row (and the mass) of a query whose own key is masked (addmask[b,P+q] <= -5000) is stored as zeros -- for hidden states of a
 * padding-free run, which carry nothing there.  Only the Q and K thirds of qkv are read; rows of probs need no alignment.
 * mtvaf_prefix_attn_mass: prefix_mass alone -- the second pass over the keys ends behind the prefix and nothing of size P+S is stored. */
int mtvaf_prefix_attn_probs(const float* qkv, const float* pk, const float* addmask, float* probs,
                            float* prefix_mass /* may be NULL */, int B, int S, int P, int NH, int head_dim,
                            int zero_masked_queries, mtvaf_stream_t stream);
int mtvaf_prefix_attn_mass(const float* qkv, const float* pk, const float* addmask, float* prefix_mass, int B, int S, int P,
                           int NH, int head_dim, int zero_masked_queries, mtvaf_stream_t stream);

/* The same attention over PACKED token rows (padding-free execution): cu [B+1] int32 -- sentence b owns rows
 * cu[b] .. cu[b+1]-1 of qkv / ctx / dctx / dqkv (its unmasked tokens in order, at most S).  Every kept key is unmasked,
 * so no additive mask is read (a masked key contributes exp(-10000) = 0 in the padded form: dropping it is exact);
 * lse / delta stay [B,NH,S].  pad_rows: the rows behind the last sentence that pad the packed image to whole tiles; an
 * extra slice of the launch zero-fills them in ctx / dqkv (an unwritten row could hold a NaN: 0 x NaN would poison dW). */
int mtvaf_prefix_attn_varlen_fwd(const float* qkv, const float* pk, const float* pv, const int* cu, int pad_rows, float* ctx,
                                 float* lse, int B, int S, int P, int NH, int head_dim, float p_drop, uint64_t seed, uint64_t offset,
                                 mtvaf_stream_t stream);
int mtvaf_prefix_attn_varlen_bwd(const float* dctx, const float* qkv, const float* pk, const float* pv, const int* cu, int pad_rows,
                                 const float* ctx, const float* lse, float* delta, float* dqkv, float* dpk, float* dpv, int B, int S,
                                 int P, int NH, int head_dim, float p_drop, uint64_t seed, uint64_t offset, mtvaf_stream_t stream);

/* Round 5, pre-split operands: the packed-row attention that ALSO writes the tile-blocked plane image of its GEMM-operand result --
 * the context as [H / 32][3][rows][32] (read by the Wo product, modeling_bert.py:353, and its weight gradient) / dQ | dK | dV as
 * [3H / 32][3][rows][32] (read by the QKV dX product and its weight gradient); rows = the packed image's row count.  Bit for bit what
 * mtvaf_f32_split_planes writes over the fp32 result, which is written as before. */
int mtvaf_prefix_attn_varlen_fwd_planes(const float* qkv, const float* pk, const float* pv, const int* cu, int pad_rows, float* ctx,
                                        float* lse, int B, int S, int P, int NH, int head_dim, float p_drop, uint64_t seed,
                                        uint64_t offset, void* ctx_planes, int rows, mtvaf_stream_t st);
int mtvaf_prefix_attn_varlen_bwd_planes(const float* dctx, const float* qkv, const float* pk, const float* pv, const int* cu, int pad_rows,
                                        const float* ctx, const float* lse, float* delta, float* dqkv, float* dpk, float* dpv, int B,
                                        int S, int P, int NH, int head_dim, float p_drop, uint64_t seed, uint64_t offset,
                                        void* dqkv_planes, int rows, mtvaf_stream_t st);
/* The packed-row attention with a per-sentence PREFIX-SLOT MASK: pmask [B, P] fp32 additive, 0 = sentence b owns slot p, -10000 = it
 * does not -- the prefix columns of the padded layout's addmask, indexed by the sentence and added at the same place of the
 * arithmetic, so a packed run with a mask equals the padded run with the same mask to the degree the unmasked runs agree.  A masked
 * slot has probability exactly 0 (exp2 underflows, as in the padded layout) and its rows of dpk / dpv are exactly 0; a sentence
 * with all P slots masked attends to its own text keys.  No tile is skipped (same products, same order).  pmask_len: the element
 * count of pmask, B * P -- anything else, or a pmask with P == 0, is MTVAF_ERR_ARG.  pmask == NULL (pmask_len ignored): the launch
 * of mtvaf_prefix_attn_varlen_fwd / _bwd.  ctx_planes / dqkv_planes with rows: as the _planes forms, or NULL for none. */
int mtvaf_prefix_attn_varlen_fwd_pm(const float* qkv, const float* pk, const float* pv, const int* cu, int pad_rows,
                                    const float* pmask, long pmask_len, float* ctx, float* lse, int B, int S, int P, int NH,
                                    int head_dim, float p_drop, uint64_t seed, uint64_t offset, void* ctx_planes, int rows,
                                    mtvaf_stream_t st);
int mtvaf_prefix_attn_varlen_bwd_pm(const float* dctx, const float* qkv, const float* pk, const float* pv, const int* cu, int pad_rows,
                                    const float* pmask, long pmask_len, const float* ctx, const float* lse, float* delta, float* dqkv,
                                    float* dpk, float* dpv, int B, int S, int P, int NH, int head_dim, float p_drop, uint64_t seed,
                                    uint64_t offset, void* dqkv_planes, int rows, mtvaf_stream_t st);
/* dst[r][:] = map[r] >= 0 ? src[map[r]][:] : 0  (rows_dst rows of H floats): packs / unpacks token rows. */
int mtvaf_gather_rows(const float* src, const int* map, float* dst, int rows_dst, int H, mtvaf_stream_t stream);
/* Token packing of a batch from its additive mask [B, T = P + S] (text keys at columns P..; kept: > -5000): cu [B+1] row
 * offsets of the sentences, inv [B*S] flat token -> packed row (-1 masked), rowmap [B*S] packed row -> flat token (-1 beyond
 * the kept rows), mv_out[0] = number of kept rows.  All int32, device. */
int mtvaf_build_packing(const float* addmask, int B, int T, int P, int S, int* cu, int* inv, int* rowmap, int* mv_out,
                        mtvaf_stream_t stream);
/* Round 6: the same with cu [2 B + 1]: behind the offsets, cu[B + 1 + z] = the sentence that the varlen attention launches
 * (mtvaf_prefix_attn_varlen_* / _bf16_varlen_*) run in slot z of their grid -- longest first -- and cu[0] = -1 marks the list as
 * present (a cu with cu[0] = 0 means sentence z in slot z).  Placement only: a launch lasts as long as its busiest CU, and in sorted
 * order the blocks a CU receives come from the long, the middle and the short third of the batch; results are bit-identical. */
int mtvaf_build_packing_ordered(const float* addmask, int B, int T, int P, int S, int* cu, int* inv, int* rowmap, int* mv_out,
                                mtvaf_stream_t stream);
/* k-tile list for mtvaf_gemm_f32_ktiles: the bk-row tiles of the [B*S] token axis that hold at least one unmasked token
 * (additive mask [B, T = P + S], kept: > -5000), in order; kcnt[0] = how many.  (B*S) % bk == 0.  Device int32 arrays. */
int mtvaf_build_ktiles(const float* addmask, int B, int T, int P, int S, int bk, int* klist, int* kcnt,
                       mtvaf_stream_t stream);
/* mtvaf_gemm_f32 for a weight-gradient product (layouts KM x KM, the reduction index is the token row) whose operand A is
 * EXACTLY ZERO outside the listed 32-row k-tiles: the reduction runs over klist[0 .. *kcnt) only (no host sync).  Gradients
 * of token rows that nothing downstream reads -- padded positions -- are exact zeros, so skipping their k-tiles changes
 * nothing but time; plans that cannot use the list reduce over the whole range (same result). */
int mtvaf_gemm_f32_ktiles(int layout_a, int layout_b, const float* A, int lda, const float* B, int ldb, float* C, int ldc,
                          int M, int N, int K, const float* bias, int epi, float* aux, int ldaux, int accumulate,
                          int allow_split, void* workspace, size_t workspace_bytes, int cfg, int splits, const int* klist,
                          const int* kcnt, mtvaf_stream_t stream);
/* p[0..n) = 0 (a kernel, not hipMemsetAsync: usable inside captured graphs, see rowops.hip). */
int mtvaf_zero_f32(float* p, long n, mtvaf_stream_t stream);

/* ---- embeddings + LayerNorm + dropout -----------------------------------------------------------------
 * replaces BertEmbeddings.forward (modeling_bert.py:212-222) / RobertaEmbeddings.forward
 * (modeling_roberta.py:102-140) and create_position_ids_from_input_ids (:1706-1719).  pos_ids == NULL
 * means arange(S) (BERT, past_key_values_length hard-coded 0 at modeling_bert.py:1050). */
int mtvaf_roberta_position_ids(const int64_t* ids, int32_t* pos_ids, int B, int S, int pad_idx, mtvaf_stream_t stream);
int mtvaf_embed_ln_fwd(const int64_t* ids, const int64_t* type_ids, const int32_t* pos_ids, const float* word,
                       const float* pos, const float* type, const float* gamma, const float* beta, float* out,
                       float* mean, float* rstd, int B, int S, int H, float eps, double p_drop, uint64_t seed,
                       uint64_t offset, void* out_bf16 /* nullable: bf16 copy of out (mixed-precision GEMM operand) */,
                       mtvaf_stream_t stream);
size_t mtvaf_embed_ln_bwd_workspace_bytes(int M, int H, int vocab, int max_pos);
int mtvaf_embed_ln_bwd(const float* dout, const int64_t* ids, const int64_t* type_ids, const int32_t* pos_ids,
                       const float* word, const float* pos, const float* type, const float* gamma, const float* mean,
                       const float* rstd, float* dword, float* dpos, float* dtype, float* dgamma, float* dbeta,
                       int accumulate, int B, int S, int H, int vocab, int max_pos, int type_vocab, int word_pad,
                       int pos_pad, double p_drop, uint64_t seed, uint64_t offset, float* dz_ws, void* workspace,
                       size_t workspace_bytes, mtvaf_stream_t stream);
/* How mtvaf_embed_ln_bwd adds token-row gradients into the word (and RoBERTa position) table: 0 (default) one owner wave per
 * table row sums its tokens in row order -- bit-reproducible; 1 float atomics (MTVAF_EMBED_ATOMIC=1).  mode 0 / 1 sets, any
 * other value queries; returns the mode in force.  (nn.Embedding's backward, modeling_bert.py:170-172.) */
int mtvaf_embed_scatter_mode(int mode);

/* ---- dropout + residual + LayerNorm --------------------------------------------------------------------
 * replaces BertSelfOutput / BertOutput `LayerNorm(dropout(dense_out) + input)` (modeling_bert.py:354-355,
 * 434-435); the dense bias is added by the GEMM epilogue.  The backward also emits the column sums of dx
 * (dbias_x, nullable) = the gradient of that dense bias, saving a separate reduction pass. */
size_t mtvaf_ln_bwd_workspace_bytes(int M, int H);
int mtvaf_dropout_res_ln_fwd(const float* x, const float* res, const float* gamma, const float* beta, float* out,
                             float* mean, float* rstd, int M, int H, float eps, double p_drop, uint64_t seed,
                             uint64_t offset, void* out_bf16 /* nullable */, mtvaf_stream_t stream);
int mtvaf_dropout_res_ln_bwd(const float* dout, const float* x, const float* res, const float* gamma,
                             const float* mean, const float* rstd, float* dx, float* dres, int dres_accumulate,
                             float* dgamma, float* dbeta, float* dbias_x, int accumulate, int M, int H, double p_drop,
                             uint64_t seed, uint64_t offset, void* workspace, size_t workspace_bytes,
                             void* dx_bf16 /* nullable: dx rounded to bf16; dx may then be NULL */, mtvaf_stream_t stream);
/* The two halves of mtvaf_dropout_res_ln_bwd as separate calls: _rows writes dx / dres and per-block partial sums into `part`
 * (mtvaf_ln_bwd_workspace_bytes(M, H) bytes, the caller's until _finish has run); _finish reduces them, in fixed order, into
 * dgamma / dbeta / dbias_x.  The layer executor runs _finish on its weight-gradient stream: the sums feed parameter
 * gradients only (autograd backward of modeling_bert.py:354-355, 434-435). */
int mtvaf_dropout_res_ln_bwd_rows(const float* dout, const float* x, const float* res, const float* gamma, const float* mean,
                                  const float* rstd, float* dx, float* dres, int dres_accumulate, int M, int H, double p_drop,
                                  uint64_t seed, uint64_t offset, float* part, void* dx_bf16 /* nullable */,
                                  mtvaf_stream_t stream);
int mtvaf_dropout_res_ln_bwd_finish(const float* part, int M, int H, float* dgamma, float* dbeta, float* dbias_x /* nullable */,
                                    int accumulate, mtvaf_stream_t stream);

/* ---- small reductions / elementwise ---------------------------------------------------------------------
 * bias gradients (column sums of dY) and nn.Dropout on the sequence output (bert_model.py:506). */
size_t mtvaf_colsum_workspace_bytes(int rows, int cols);
int mtvaf_colsum(const float* x, int rows, int cols, int ld, float* out, int accumulate, void* workspace,
                 size_t workspace_bytes, mtvaf_stream_t stream);
/* p_drop is a double: kept elements are scaled by float(1 / (1 - p)) as torch scales them (in fp32 from a float p that is
 * 9.999998, not 10, at p = 0.9). */
int mtvaf_dropout(const float* x, float* y, long n, double p_drop, uint64_t seed, uint64_t offset,
                  mtvaf_stream_t stream);

/* ---- linear-chain CRF head --------------------------------------------------------------------------------
 * replaces torchcrf.CRF(num_tags, batch_first=True): forward(..., reduction='mean') negated at
 * bert_model.py:521 and decode at :511.  emissions [B,S,C], tags int64 [B,S], mask uint8 [B,S] with
 * mask[:,0] == 1, 1 <= C <= 64; for 16 < C <= 64 also S <= 512.  Other shapes: MTVAF_ERR_SHAPE before any
 * launch, and mtvaf_crf_workspace_bytes returns 0.  loss[0] = -mean_b(score(gold) - logZ).  The workspace
 * written by the forward is read by the backward.  tags_out int32 [B,S] (-1 padded), lens_out int32 [B]. */
size_t mtvaf_crf_workspace_bytes(int B, int S, int C);
int mtvaf_crf_nll_fwd(const float* emissions, const int64_t* tags, const uint8_t* mask, const float* start,
                      const float* end, const float* trans, float* loss, int B, int S, int C, void* workspace,
                      size_t workspace_bytes, mtvaf_stream_t stream);
int mtvaf_crf_nll_bwd(const float* grad_out, const float* emissions, const int64_t* tags, const uint8_t* mask,
                      const float* start, const float* end, const float* trans, float* demissions, float* dstart,
                      float* dend, float* dtrans, int accumulate, int B, int S, int C, void* workspace,
                      size_t workspace_bytes, mtvaf_stream_t stream);
int mtvaf_crf_viterbi(const float* emissions, const uint8_t* mask, const float* start, const float* end,
                      const float* trans, int32_t* tags_out, int32_t* lens_out, int B, int S, int C,
                      mtvaf_stream_t stream);

/* per-sentence likelihoods and tag marginals: same shapes, error codes and workspace (mtvaf_crf_workspace_bytes) as
 * the entry points above; no host sync, no allocation, safe under stream capture.
 *   llh_fwd   llh[b] = score(gold_b) - logZ_b (torchcrf's sign); leaves in the workspace what llh_bwd reads.
 *   llh_bwd   grad_llh [B] = d(total)/d(llh[b]): demissions[b,t,:] = grad_llh[b] (onehot(gold) - marginal) at unmasked
 *             steps, exact zeros at masked ones; dstart/dend/dtrans = sum_b grad_llh[b] d(llh[b])/d(.), overwritten
 *             or accumulated.
 *   marginals marg[b,t,j] = p(y_t = j | emissions_b) at unmasked steps, exact zeros at masked ones (holes included);
 *             takes no tags; logz [B] may be NULL.  Overwrites the workspace of a preceding forward. */
int mtvaf_crf_llh_fwd(const float* emissions, const int64_t* tags, const uint8_t* mask, const float* start,
                      const float* end, const float* trans, float* llh, int B, int S, int C, void* workspace,
                      size_t workspace_bytes, mtvaf_stream_t stream);
int mtvaf_crf_llh_bwd(const float* grad_llh, const float* emissions, const int64_t* tags, const uint8_t* mask,
                      const float* start, const float* end, const float* trans, float* demissions, float* dstart,
                      float* dend, float* dtrans, int accumulate, int B, int S, int C, void* workspace,
                      size_t workspace_bytes, mtvaf_stream_t stream);
int mtvaf_crf_marginals(const float* emissions, const uint8_t* mask, const float* start, const float* end,
                        const float* trans, float* marg, float* logz, int B, int S, int C, void* workspace,
                        size_t workspace_bytes, mtvaf_stream_t stream);

/* n-best Viterbi: the K best tag sequences of every sentence, 1 <= K <= 8, 1 <= C <= 64, 1 <= S <= 512 (anything else:
 * MTVAF_ERR_SHAPE before any launch, and the workspace query returns 0; a workspace below the query: MTVAF_ERR_WORKSPACE).
 * mask is a prefix mask with mask[:,0] == 1: len_b = its leading ones, end[] is added at step len_b - 1.
 *   tags_out    int32 [B,K,S]: row k the k-th best path in columns < len_b, -1 behind it
 *   scores_out  [B,K] unnormalised path scores (the terms of llh_fwd's gold-path score), non-increasing in k
 *   logprob_out [B,K] = score - logZ_b, logZ by the forward recursion of mtvaf_crf_marginals; NULL: not computed, no forward launch
 *   n_paths_out int32 [B] = min(K, C^len_b); ranks >= n_paths: tags -1, score and log-probability -inf.
 * Equal scores: the lower previous tag first, then the lower previous rank; at the end the lower last tag, then the lower rank
 * (rank 0 follows mtvaf_crf_viterbi's rule).  workspace bytes: round256(2 B S K C) back-pointers + round256(4 B) logZ +
 * mtvaf_crf_workspace_bytes(B, S, C).  No host sync, no allocation; safe under stream capture. */
size_t mtvaf_crf_nbest_workspace_bytes(int B, int S, int C, int K);
int mtvaf_crf_nbest(const float* emissions, const uint8_t* mask, const float* start, const float* end, const float* trans,
                    int K, int32_t* tags_out, float* scores_out, float* logprob_out, int32_t* n_paths_out, int B, int S,
                    int C, void* workspace, size_t workspace_bytes, mtvaf_stream_t stream);

/* Posterior sampling (csrc/crf_sample.hip): K tag sequences of every sentence drawn from p(y | x) by forward-filter
 * backward-sample, 1 <= K <= 64, 1 <= C <= 64, 1 <= S <= 512 (anything else: MTVAF_ERR_SHAPE before any launch, and the
 * workspace query returns 0; a workspace below the query: MTVAF_ERR_WORKSPACE).  mask is a prefix mask with mask[:,0] == 1, as
 * for mtvaf_crf_nbest.  The forward recursion is mtvaf_crf_marginals' first launch; its alphas are read from the workspace.
 * Sample k of sentence b, columns t = len_b - 1 .. 0:  x_i = log alpha_t[i] + (t == len_b - 1 ? end[i] : trans[i][y_{t+1}]),
 * w_i = exp(x_i - max_i x_i), F_j = sum_{i <= j} w_i in ascending tag order in fp32; y_t = the smallest j with
 * F_j > u * F_{C-1}; if rounding leaves none, the highest j with w_j > 0.
 *   uniforms     [B,K,S] fp32 in [0,1): u of (b, k, t) is read here; NULL: Philox4x32-10 with counter (lo32(idx), hi32(idx),
 *                lo32(offset), hi32(offset)), idx = (b * 64 + k) * 128 + (t >> 2), key (lo32(seed), hi32(seed)), word t & 3,
 *                u = (word >> 8) * 2^-24; offset takes the dropout epoch (mtvaf_rng_set_epoch_ptr) like a dropout site
 *   tags_out     int32 [B,K,S]: sample k in columns < len_b, -1 behind it
 *   scores_out   [B,K] unnormalised path scores (the terms of mtvaf_crf_nbest's scores_out)
 *   logprob_out  [B,K] = score - logZ_b, or NULL
 *   uniforms_out [B,K,S] the uniform used at every column < len_b, 0 behind it, or NULL
 * Every element of every non-NULL output is written.  workspace bytes: round256(4 B) logZ + mtvaf_crf_workspace_bytes(B, S, C).
 * No host sync, no allocation; safe under stream capture (the forward's LDS opt-in for C <= 16 and S above about 470: as
 * mtvaf_crf_marginals). */
size_t mtvaf_crf_sample_workspace_bytes(int B, int S, int C, int K);
int mtvaf_crf_sample(const float* emissions, const uint8_t* mask, const float* start, const float* end, const float* trans,
                     int K, const float* uniforms, uint64_t seed, uint64_t offset, int32_t* tags_out, float* scores_out,
                     float* logprob_out, float* uniforms_out, int B, int S, int C, void* workspace, size_t workspace_bytes,
                     mtvaf_stream_t stream);

/* per-token tag constraints (csrc/crf_lattice.hip): likelihood, posteriors and decoding over the paths a per-position tag
 * set allows.  allowed int64 [B,S], read as an unsigned word: bit j set = tag j may be taken at that column.  The effective
 * set is A[b,t] = allowed[b,t] & (2^C - 1), and the full set where that is empty (0 = no constraint, bits >= C ignored), so
 * every input has a finite answer and nothing is checked on the host.  1 <= C <= 64, 1 <= S <= 512 (anything else:
 * MTVAF_ERR_SHAPE before any launch, and the workspace query returns 0; a workspace below the query: MTVAF_ERR_WORKSPACE).
 * mask is a prefix mask with mask[:,0] == 1: len_b = its leading ones, columns at or beyond len_b are never read, end[]
 * enters at column len_b - 1.  score(y) is llh_fwd's path score; logZ_A[b] = log sum_{y: y_t in A[b,t]} exp score(y).
 *   lattice_fwd        pllh[b] = logZ_A[b] - logZ[b] <= 0; logz_a [B] and logz [B] may be NULL; leaves in the workspace what
 *                      lattice_bwd reads.
 *   lattice_bwd        gradients of sum_b grad[b] pllh[b]: demissions[b,t,:] = grad[b] (muA - mu) at unmasked columns, exact
 *                      zeros at masked ones; dstart/dend/dtrans from the two sets of node and edge marginals, overwritten
 *                      or accumulated as by llh_bwd.
 *   lattice_marginals  marg[b,t,j] = muA, the posterior under the constraint: exact zeros at disallowed tags and masked
 *                      columns; logz_a [B] may be NULL.  Overwrites the workspace of a preceding lattice_fwd.
 *   lattice_viterbi    tags_out int32 [B,S] the best allowed path (-1 behind len_b), lens_out int32 [B] = len_b, score_out [B]
 *                      (may be NULL) its unnormalised score.  Ties: the lowest allowed previous tag, at the end the lowest
 *                      allowed last tag; mtvaf_crf_viterbi's order of additions, so full sets give its output bit for bit.
 * A sentence whose effective sets are all full has pllh[b] == +0.0 and contributes exact zeros to every gradient.  The
 * constrained chain takes its per-step maximum over the allowed tags only: finite inputs give finite results however far
 * the allowed emissions lie below the others.  No host sync, no allocation; safe under single-stream capture. */
size_t mtvaf_crf_lattice_workspace_bytes(int B, int S, int C);
int mtvaf_crf_lattice_fwd(const float* emissions, const int64_t* allowed, const uint8_t* mask, const float* start,
                          const float* end, const float* trans, float* pllh, float* logz_a, float* logz, int B, int S,
                          int C, void* workspace, size_t workspace_bytes, mtvaf_stream_t stream);
int mtvaf_crf_lattice_bwd(const float* grad, const float* emissions, const int64_t* allowed, const uint8_t* mask,
                          const float* start, const float* end, const float* trans, float* demissions, float* dstart,
                          float* dend, float* dtrans, int accumulate, int B, int S, int C, void* workspace,
                          size_t workspace_bytes, mtvaf_stream_t stream);
int mtvaf_crf_lattice_marginals(const float* emissions, const int64_t* allowed, const uint8_t* mask, const float* start,
                                const float* end, const float* trans, float* marg, float* logz_a, int B, int S, int C,
                                void* workspace, size_t workspace_bytes, mtvaf_stream_t stream);
int mtvaf_crf_lattice_viterbi(const float* emissions, const int64_t* allowed, const uint8_t* mask, const float* start,
                              const float* end, const float* trans, int32_t* tags_out, int32_t* lens_out, float* score_out,
                              int B, int S, int C, mtvaf_stream_t stream);

/* expected cost (risk) under the chain's posterior and its gradients (csrc/crf_risk.hip) -- the losses that need the gradient
 * of a posterior expectation, which the reference's CRF (models/bert_model.py:464, :521: log-likelihood only) cannot train:
 * expected Hamming / cost-sensitive risk, distillation on marginals, and the vector-Jacobian product of the node marginals.
 * cost fp32 [B,S,C], additive over columns: risk[b] = E_{y ~ p(.|x_b)} sum_{t < len_b} cost[b,t,y_t].  1 <= C <= 64,
 * 1 <= S <= 512 (anything else: MTVAF_ERR_SHAPE before any launch, and the workspace query returns 0; a workspace below the
 * query: MTVAF_ERR_WORKSPACE).  mask is a prefix mask with mask[:,0] == 1: len_b = its leading ones; emissions and cost at or
 * beyond len_b are never read (they may hold NaN), end[] enters at column len_b - 1.
 *   risk_fwd  risk [B]; logz [B] (the log-partition) and marg [B,S,C] (the node marginals m_t(c), zeros at masked columns) may
 *             be NULL; one launch, two with marg.  Leaves in the workspace what risk_bwd reads.
 *   risk_bwd  gradients of sum_b grad[b] risk[b] after a risk_fwd on the same inputs and workspace:
 *             demissions[b,t,c] = grad[b] m_t(c) (E[cost | y_t = c] - risk[b]), dcost[b,t,c] = grad[b] m_t(c) (dcost may be NULL),
 *             exact zeros at masked columns; dstart / dend / dtrans from the same covariances on the edge marginals, reduced
 *             over sentences in a fixed order, overwritten or accumulated as by llh_bwd.  Two launches.
 * The recursions are re-centred at every step (the conditional expectations never grow with the length), so the float32
 * error of a gradient does not grow with len |cost|.  sum_c demissions[b,t,c] = 0 up to rounding; a constant added to
 * cost[b,t,:] moves risk[b] by it and no gradient.  Exact zeros, all written as +0.0 whatever the sign of grad[b]: cost == 0 on
 * the live columns gives risk == 0 and zero gradients; grad[b] == 0 gives zeros for that sentence.  The vector-Jacobian product of the marginals with a cotangent V
 * [B,S,C] is risk_fwd + risk_bwd with cost = V and grad = 1.  Results are bit-reproducible.  No host sync, no allocation,
 * no atomics; safe under single-stream capture. */
size_t mtvaf_crf_risk_workspace_bytes(int B, int S, int C);
int mtvaf_crf_risk_fwd(const float* emissions, const float* cost, const uint8_t* mask, const float* start, const float* end,
                       const float* trans, float* risk, float* logz, float* marg, int B, int S, int C, void* workspace,
                       size_t workspace_bytes, mtvaf_stream_t stream);
int mtvaf_crf_risk_bwd(const float* grad, const float* emissions, const float* cost, const uint8_t* mask, const float* start,
                       const float* end, const float* trans, float* demissions, float* dcost, float* dstart, float* dend,
                       float* dtrans, int accumulate, int B, int S, int C, void* workspace, size_t workspace_bytes,
                       mtvaf_stream_t stream);

/* expected PATH cost with a term on every edge, and its gradients (csrc/crf_path.hip) -- crf_risk with one more term per
 * previous tag; with it the sequence entropy, the KL divergence between two chains and the edge marginals.
 * cost fp32 [B,S,C] or NULL, ecost fp32 [C,C] or NULL (NULL reads as zeros):
 *   W(y) = sum_{t < len_b} cost[b,t,y_t] + sum_{1 <= t < len_b} ecost[y_{t-1},y_t],   risk[b] = E_{y ~ p(.|x_b)} W(y).
 * Limits and error behaviour are those of mtvaf_crf_risk_*: 1 <= C <= 64, 1 <= S <= 512 (anything else: MTVAF_ERR_SHAPE before
 * any launch, and the workspace query returns 0; a workspace below the query: MTVAF_ERR_WORKSPACE); a prefix mask with
 * mask[:,0] == 1; emissions and cost at or beyond len_b are never read (they may hold NaN).
 *   path_fwd  risk [B]; logz [B] may be NULL; one launch.  Leaves in the workspace what path_bwd reads.
 *   path_bwd  the gradients of sum_b grad[b] risk[b] + gz[b] logZ[b] (gz [B] or NULL = zeros), with cost and ecost those of
 *             the forward call: demissions = grad dR/dem + gz m_t(c); dcost (or NULL) = grad m_t(c); decost [C,C] (or NULL) =
 *             sum_b grad[b] sum_t xi_t(i,j); dstart / dend / dtrans the cost covariances on the end-point and edge marginals
 *             under grad plus those marginals themselves under gz; the parameter gradients and decost are reduced over
 *             sentences in a fixed order, overwritten or accumulated.  Two launches.
 * The recursions are centred as crf_risk's.  Exact zeros, all written as +0.0: masked columns of demissions and dcost; a
 * sentence with grad[b] == 0 and gz[b] == 0; every cost-covariance gradient (and risk) when cost and ecost are both zero or
 * NULL.  Both costs NULL with gz = w gives w times the gradient of logZ.  Results are bit-reproducible.  No host sync, no
 * allocation, no atomics; safe under single-stream capture. */
size_t mtvaf_crf_path_workspace_bytes(int B, int S, int C);
int mtvaf_crf_path_fwd(const float* emissions, const float* cost, const float* ecost, const uint8_t* mask, const float* start,
                       const float* end, const float* trans, float* risk, float* logz, int B, int S, int C, void* workspace,
                       size_t workspace_bytes, mtvaf_stream_t stream);
int mtvaf_crf_path_bwd(const float* grad, const float* gz, const float* emissions, const float* cost, const float* ecost,
                       const uint8_t* mask, const float* start, const float* end, const float* trans, float* demissions,
                       float* dcost, float* decost, float* dstart, float* dend, float* dtrans, int accumulate, int B, int S,
                       int C, void* workspace, size_t workspace_bytes, mtvaf_stream_t stream);

/* ---- visual prompt generator + VAO loss ----------------------------------------------------------------------
 * replaces TVNetSAModel2.get_visual_prompt's split-mean / gates / gated sums / cat / reshape
 * (bert_model.py:544-545, 566-585) and the KLDiv(batchmean) ANP loss (:549-563).
 * enc [NI,B,L,4W] (encoder_conv output, NI = 1+n_aux), sm [NI*B,L*W], gate/logits [NI*B,NL*4],
 * pkv [NL,2,B,(NI*L)*(W/2)] -- the slabs mtvaf_prefix_attn_* read. */
int mtvaf_split_mean(const float* enc, float* sm, long rows, int W, mtvaf_stream_t stream);
int mtvaf_gate_fwd(const float* logits, float* gate, long ngroups, mtvaf_stream_t stream);
int mtvaf_prompt_mix_fwd(const float* enc, const float* gate, float* pkv, int NI, int B, int L, int W, int NL,
                         mtvaf_stream_t stream);
int mtvaf_prompt_mix_bwd_gate(const float* enc, const float* dpkv, const float* logits, const float* gate,
                              float* dgate_part, float* dlogits, int NI, int B, int L, int W, int NL,
                              mtvaf_stream_t stream);
int mtvaf_prompt_mix_bwd_enc(const float* gate, const float* dpkv, const float* dsm, float* denc, int NI, int B,
                             int L, int W, int NL, mtvaf_stream_t stream);
int mtvaf_kl_logsoftmax_fwd(const float* logits, const float* target, float* loss, float* row_ws, int B, int N,
                            mtvaf_stream_t stream);
/* The same loss over the rows that are PRESENT (present [B] fp32, 1 / 0: the sentences that have this image): loss[0] = sum over
 * present rows of the row's KL term / the number of present rows (0 when none is); an absent row adds nothing and gets a zero
 * gradient.  All rows present: the bits of mtvaf_kl_logsoftmax_fwd / _bwd (the same sums in the same order, factor B / B = 1). */
int mtvaf_kl_logsoftmax_masked_fwd(const float* logits, const float* target, const float* present, float* loss, float* row_ws,
                                   int B, int N, mtvaf_stream_t stream);
int mtvaf_kl_logsoftmax_masked_bwd(const float* grad_out, float gscale, const float* logits, const float* target,
                                   const float* present, float* dlogits, int B, int N, mtvaf_stream_t stream);
int mtvaf_kl_logsoftmax_bwd(const float* grad_out, float gscale, const float* logits, const float* target,
                            float* dlogits, int B, int N, mtvaf_stream_t stream);
int mtvaf_mean_l_fwd(const float* enc, float* out, long n, int L, int W4, mtvaf_stream_t stream);
int mtvaf_mean_l_bwd(const float* dmean, float* denc, long n, int L, int W4, mtvaf_stream_t stream);

/* ---- span model heads: TVNetSAModel.classification + the loss of TVNetSAModel.forward --------------------------
 * Replaces models/bert_model.py:140-179 (flatten_emb_by_sentence, get_span_representation,
 * get_self_att_representation), :181-190 (distant_cross_entropy), :288-303 (CrossEntropyLoss on the span logits).
 * mask [B,S] u8, span_starts/ends [B,M] int64 (token offsets inside each sentence), seq [B*S,H] fp32 (H % 4 == 0,
 * H <= 1024).  `index` is a device int32 block of mtvaf_span_index_ints(B,S,M) entries that mtvaf_span_index fills
 * (valid-token compaction, per-span offsets/widths, text length and JR = widest span, clamped to S) -- the sizes
 * the reference reads back to the host stay on the device.  pooled [B*M,H], stats [B*M,2].
 * Contract: 0 <= span_starts, span widths <= S.  A wider span is truncated: JR = min(widest span, S), and pooled is
 * what the reference returns with every span's end cut to start + S - 1 (the reference would index past S only for
 * spans that leave the sentence).  rowmap is specified in its first text_length entries only. */
size_t mtvaf_span_index_ints(int B, int S, int M);
int mtvaf_span_index(const uint8_t* mask, const int64_t* span_starts, const int64_t* span_ends, int* index, int B,
                     int S, int M, mtvaf_stream_t stream);
int mtvaf_span_pool_fwd(const float* seq, const float* w_unary, const float* b_unary, const int* index,
                        float* pooled, float* stats, int B, int S, int M, int H, mtvaf_stream_t stream);
size_t mtvaf_span_pool_bwd_workspace_bytes(int B, int S, int M, int H);
/* dseq [B*S,H] overwritten (deterministic, no atomics); *dw_part_out [B*M,H] / *db_part_out [B*M] point into the
 * workspace: their column sums (mtvaf_colsum) are the unary_affine weight / bias gradients. */
int mtvaf_span_pool_bwd(const float* dpooled, const float* pooled, const float* stats, const float* seq,
                        const float* w_unary, const float* b_unary, const int* index, float* dseq,
                        float** dw_part_out, float** db_part_out, int B, int S, int M, int H, void* ws,
                        size_t ws_bytes, mtvaf_stream_t stream);
/* loss (+)= scale * -mean_b( sum_s pos log_softmax(logits)_s / sum_s pos );  logits element (b,s) at
 * logits[(b*S+s)*ld] (the start / end logits are the two columns of the binary_affine output, ld = 2);
 * positions [B,S] fp32 multi-hot; row_ws [B,3] = (row value, log sum_s exp(logit - row max), sum_s pos) is kept for
 * the backward, which finds the row maximum again: a common offset of a row's logits does not cost precision. */
int mtvaf_distant_ce_fwd(const float* logits, int ld, const float* positions, float* loss, float* row_ws, int B,
                         int S, float scale, int accumulate, mtvaf_stream_t stream);
int mtvaf_distant_ce_bwd(const float* grad_out, float scale, const float* logits, int ld, const float* positions,
                         const float* row_ws, float* dlogits, int ldd, int B, int S, mtvaf_stream_t stream);
/* mean cross entropy over rows with label != -100 (C <= 64); ws2 [2] is kept for the backward. */
int mtvaf_ce_fwd(const float* logits, const int64_t* labels, float* loss, float* ws2, int N, int C,
                 mtvaf_stream_t stream);
int mtvaf_ce_bwd(const float* grad_out, const float* logits, const int64_t* labels, const float* ws2,
                 float* dlogits, int N, int C, mtvaf_stream_t stream);
/* Cutoff consistency term of the span model (modules/train.py:523-538, cal_cut_loss / js_div): x, y [B,M,C] fp32
 * contiguous, the polarity logits of the plain and of the cut pass.  The softmax runs over axis 1, the M candidate slots,
 * separately for every (b,c) column -- the reference's dim=1 on [B,M,4].  With p = softmax_m(x), q = softmax_m(y),
 * mbar = (p+q)/2:
 *   loss[0] = scale / (2B) * sum_{b,m,c} mbar (2 log mbar - log p - log q)
 * which is the value of js_div: (KL(mbar||p) + KL(mbar||q)) / 2 under kl_div's 'batchmean'.  The KLs run FROM mbar, so
 * this is not the textbook Jensen-Shannon divergence: it is >= 0 and unbounded.  The reference's +1e-10 on the logits
 * is dropped (softmax is shift-invariant).  Evaluated in log space with expf / logf / log1pf, so probabilities that
 * underflow give finite values and gradients where the reference's fp32 form gives NaN.
 * mask [B,M] u8 or NULL (an extension; NULL = the reference: padding slots take part): slots with mask 0 are left out of
 * both softmaxes and of the sum, their dx / dy entries are exact 0; a sentence without a live slot adds 0; the divisor
 * stays B.  row_ws [B] is scratch.  The backward recomputes everything from x, y and mask (nothing is kept from the
 * forward): dx, dy [B,M,C] = *grad_out (device) times the gradient of loss[0], through p, q and mbar, every element
 * written.  No floating-point atomics: the same inputs give the same bits.  B >= 1, 1 <= M <= 1024, 1 <= C <= 16
 * (MTVAF_ERR_SHAPE, checked before any launch). */
int mtvaf_js_consistency_fwd(const float* x, const float* y, const uint8_t* mask, float* loss, float* row_ws, int B,
                             int M, int C, float scale, mtvaf_stream_t stream);
int mtvaf_js_consistency_bwd(const float* grad_out, float scale, const float* x, const float* y, const uint8_t* mask,
                             float* dx, float* dy, int B, int M, int C, mtvaf_stream_t stream);
/* Token-level divergence between the emissions of two passes over one batch -- the consistency term of R-Drop and of a
 * plain / cut pair for the tagger (csrc/consistency.hip).  x, y [N,C] fp32 contiguous, N = B*S rows
 * (they may be the same buffer: the value is then exactly 0); mask [N] u8 (non-zero = live) or NULL = every row live.  Per
 * live row, with u = x/T, v = y/T (T = temperature), lp = log_softmax(u), lq = log_softmax(v), p = exp(lp), q = exp(lq):
 *   kind 0 (symmetric KL)     L = 1/2 sum_c (p_c - q_c)(lp_c - lq_c)                      >= 0, unbounded
 *   kind 1 (Jensen-Shannon)   L = 1/2 sum_c p_c (lp_c - lm_c) + 1/2 sum_c q_c (lq_c - lm_c),  lm = log((p + q) / 2);  0 <= L <= log 2
 *   loss[0] = scale * (sum of L over the live rows) / D
 * reduction 0 (token mean): D = the number of live rows, counted on the device; D = 0 gives loss 0 and all-zero gradients.
 * reduction 1 (batch mean): D = B (B is read in this mode only).  row_ws [N] receives every row's L, 0 on masked rows.
 * The backward recomputes everything from x, y and mask (nothing is kept from the forward) and writes every element of
 * dx, dy [N,C], exact zeros on masked rows:  with d = lp - lq, A = sum_c p_c d_c, a = lp - lm, Abar = sum_c p_c a_c
 *   kind 0   dL/du_c = 1/2 [p_c (d_c - A) + p_c - q_c]        kind 1   dL/du_c = 1/2 p_c (a_c - Abar)
 *   dL/dx = dL/du / T, the y side with the roles swapped, all of it times *grad_out (device) * scale / D.
 * Contract: evaluated in log space with the row maximum removed -- logits of magnitude 1e4 and rows whose two distributions
 * put all mass on different tags give a finite value and finite gradients (kind 0), a value <= log 2 (kind 1); masked rows
 * are never read and may hold NaN; no floating-point atomics -- the row values are added in double in a fixed order by one
 * finishing block, so the same inputs give the same bits; no host sync, no read-back.  N >= 1, 1 <= C <= 64
 * (MTVAF_ERR_SHAPE); kind and reduction 0 or 1, finite temperature > 0, B >= 1 with reduction 1, no NULL but mask
 * (MTVAF_ERR_ARG); all checked before any launch. */
int mtvaf_token_divergence_fwd(const float* x, const float* y, const uint8_t* mask, float* loss, float* row_ws, int N,
                               int C, int kind, float temperature, int reduction, int B, float scale,
                               mtvaf_stream_t stream);
int mtvaf_token_divergence_bwd(const float* grad_out, const float* x, const float* y, const uint8_t* mask, float* dx,
                               float* dy, int N, int C, int kind, float temperature, int reduction, int B, float scale,
                               mtvaf_stream_t stream);
/* Token-level cross entropy over the tagger's emissions -- the loss of a softmax tagging head and the auxiliary term beside
 * the CRF, with class weights, label smoothing and the focal factor (csrc/token_ce.hip).
 * logits [N,C] fp32 contiguous, N = B*S rows; labels [N] int64; mask [N] u8 (non-zero = live) or NULL; class_weight w [C]
 * fp32 or NULL = all ones.  A row is LIVE iff its mask byte is non-zero (or mask is NULL), its label is not ignore_index
 * and its label lies in [0, C); a label outside [0, C) that is not ignore_index on an unmasked row makes the row dead and is
 * counted in stats[1] (the label of a masked row is not looked at).  Per live row with label y, lp = log_softmax(z),
 * p = exp(lp), eps = smoothing, g = gamma:
 *   a_c = (1 - eps) w_y [c = y] + (eps / C) w_c          A = sum_c a_c
 *   ce  = -sum_c a_c lp_c       om = sum_{c != y} p_c  (= 1 - p_y, formed as this sum)       L = om^g ce   (g = 0: L = ce)
 *   dL/dz_k = om^g (A p_k - a_k) - ce g om^(g-1) p_y ([k = y] - p_k)
 *   loss[0] = scale * (sum of L over the live rows) / D
 * reduction 0 (mean): D = sum of w_y over the live rows -- at g = 0 torch.nn.functional.cross_entropy(weight=,
 * label_smoothing=, ignore_index=); D = 0 gives loss 0 and all-zero gradients.  reduction 1 (batch mean): D = B (read in
 * this mode only; commensurable with the CRF's mean NLL).  reduction 2 (sum): D = 1.  row_ws [N] receives every row's L,
 * exactly 0 on dead rows; stats [2] int32 receives the number of live rows and of out-of-range labels.
 * The backward recomputes everything from its inputs (nothing is kept from the forward) and writes every element of
 * dlogits [N,C], exact zeros on dead rows: dL/dz times *grad_out (device) * scale / D -- or, with grad_rows [N] in place of
 * grad_out (exactly one of the two is given), times scale * grad_rows[row], the per-row upstream gradient of the rows
 * themselves (reduction and B are then not read; grad_rows is not read on dead rows).
 * Contract: log space with the row maximum removed -- logits of magnitude 1e4 give finite values and gradients, and a row
 * whose other tags all underflow has om = 0 exactly, so its focal value and gradient are exact zeros; dead rows are never
 * read and may hold NaN; no floating-point atomics -- one finishing block adds the rows and D in double in a fixed order
 * (the backward forms D the same way in every block), so the same inputs give the same bits; no host sync, no read-back,
 * no LDS opt-in.  N >= 1, 1 <= C <= 64 (MTVAF_ERR_SHAPE); smoothing in [0, 1), gamma 0 or in [1, 8], reduction 0..2,
 * B >= 1 with reduction 1, no NULL but mask, class_weight and one of grad_out / grad_rows (MTVAF_ERR_ARG); all checked
 * before any launch. */
int mtvaf_token_ce_fwd(const float* logits, const int64_t* labels, const uint8_t* mask, const float* class_weight,
                       float* loss, float* row_ws, int* stats, int N, int C, long ignore_index, float smoothing,
                       float gamma, int reduction, int B, float scale, mtvaf_stream_t stream);
int mtvaf_token_ce_bwd(const float* grad_out, const float* grad_rows, const float* logits, const int64_t* labels,
                       const uint8_t* mask, const float* class_weight, float* dlogits, int N, int C, long ignore_index,
                       float smoothing, float gamma, int reduction, int B, float scale, mtvaf_stream_t stream);
/* Per-token decoding of a softmax head (csrc/token_ce.hip).  tags [N] int64 = the first maximum of each live row of
 * logits [N,C]; logp [N] = log_softmax at it, taken over all C tags.  mask [N] u8 or NULL; masked rows are not read and get
 * tag 0 and logp 0.  allowed [N] int64 or NULL: tag sets in the format of the constrained CRF entry points (bit j = tag j
 * permitted; a word without any of the low C bits = no constraint): the maximum runs over the permitted tags only, logp
 * stays the unconstrained log-probability.  N >= 1, 1 <= C <= 64 (MTVAF_ERR_SHAPE); no NULL but mask and allowed
 * (MTVAF_ERR_ARG). */
int mtvaf_token_argmax(const float* logits, const uint8_t* mask, const int64_t* allowed, int64_t* tags, float* logp, int N,
                       int C, mtvaf_stream_t stream);
/* Candidate spans at eval / predict time: the eval branch of models/utils.py::span_annotate_candidates (:451-521) and
 * the host round trip around it (modules/train.py:382-410) as one launch, no host read-back.  Start logit of (b,s) at
 * logits[(b*S+s)*ld], end logit one element later (the binary_affine output, ld = 2).  word_index [B,S] int32: token
 * -> original word, -1 outside the reference's token_to_orig_map; word_key [B,S] int32 or NULL: an id of the word's
 * string (equal strings, equal ids); NULL = word_index (positional de-duplication).  Per sentence: the top
 * min(n_best,S) start and end positions (logit descending, position ascending, masked positions included), their
 * pairs in that order with both ends in the map, e >= s, e-s+1 <= max_len and (double)sl+(double)el >= threshold,
 * ordered by key = that fp64 sum [- (e-s+1) with use_heuristics] descending, pair order ascending; walked greedily
 * until 2*accepted >= n_best, skipping a pair whose word-key signature equals an accepted span's (nms = 1: that
 * shares any word key with one).  span_starts / span_ends / label_masks [B,n_best] int64 and span_scores [B,n_best]
 * fp32 (the fp64 sum rounded) are zero-padded, count [B] int32; every element is written.  1 <= S <= 512,
 * 1 <= n_best <= 32.  Contract: finite logits; word_index rises by 0 or 1 along each run of in-map tokens. */
int mtvaf_span_propose(const float* logits, int ld, const int* word_index, const int* word_key,
                       int64_t* span_starts, int64_t* span_ends, int64_t* label_masks, float* span_scores, int* count,
                       int B, int S, int n_best, int max_len, float threshold, int use_heuristics, int nms,
                       mtvaf_stream_t stream);

/* Entity-level score of decoded tags, the counting half: what modules/train.py:627-647 / :714-731 (y_true / y_pred on the
 * host), modules/eval_metrics.py::get_chunks / evaluate / evaluate_each_class and seqeval's classification_report count,
 * ADDED into a device counter by one launch with no host read-back.  pred [B,ldp] int32 (mtvaf_crf_viterbi's tags, -1
 * beyond each length; ldp >= S), gold [B,S] int64, mask [B,S] u8.  Kept columns of a sentence: 1 .. S-1 while mask is 1
 * (up to the first 0), minus those with gold_skip[gold] set ([C] u8); a label id outside [0,C) reads as 0.  The tagging
 * scheme is the two tables start_tab / end_tab [(C+1)*(C+1)] u8 indexed [prev*(C+1)+cur], index C = sentence boundary:
 * per side, over the kept labels l_j, a start at j iff start_tab[l_j-1][l_j], an end at j iff end_tab[l_j][l_j+1]; every
 * end closes one chunk (type_of[l_j], b, j) with b the greatest start <= j of the sentence (none: the chunk is unopened,
 * counted for its type, never correct).  type_of [C+1] int32 in [0,n_types).  counts [n_types*3+2] int64: per type
 * predicted, gold, correct (both sides end at j with the same opened b and the same type), then tokens_equal, tokens_kept.
 * Integer atomics only: bit-reproducible.  1 <= S <= 512, 1 <= C <= 64, 1 <= n_types <= C+1. */
int mtvaf_entity_counts(const int* pred, int ldp, const int64_t* gold, const uint8_t* mask, const uint8_t* start_tab,
                        const uint8_t* end_tab, const int* type_of, const uint8_t* gold_skip, int B, int S, int C,
                        int n_types, int64_t* counts, mtvaf_stream_t stream);

/* The same chunking per row: rows_out int32 [R,3] = (predicted, gold, correct) chunks of row r summed over the types; every
 * element is written and nothing is added anywhere.  pred [R,ldp] int32; row r is scored against gold / mask row r / group
 * (gold and mask [R/group,S]), so hypotheses [B,K,S] go in as R = B K, group = K.  Kept columns, tables, gold_skip and shape
 * rules as mtvaf_entity_counts, plus group >= 1 and R % group == 0 (else MTVAF_ERR_SHAPE before any launch). */
int mtvaf_entity_counts_rows(const int* pred, int ldp, int group, const int64_t* gold, const uint8_t* mask,
                             const uint8_t* start_tab, const uint8_t* end_tab, const int* type_of, const uint8_t* gold_skip,
                             int R, int S, int C, int n_types, int32_t* rows_out, mtvaf_stream_t stream);

/* Aspect-level score of the span model's predictions, the counting of modules/eval_metrics.py::eval_absa (:80-124) without
 * the per-sentence host copies of modules/train.py:200-209: common / retrieved / relevant per polarity class, ADDED into a
 * device counter by one launch with no host read-back.  Integers only, apart from one arg-max over fp32.
 * span_starts / span_ends / label_masks [B,N] int64 as mtvaf_span_propose writes them, logits [B,N,K] fp32 (the polarity
 * logits of every slot); gold_starts / gold_ends / gold_class / gold_masks [B,G] int64 (the feature's start_indexes,
 * end_indexes, polarity_labels, label_masks: models/utils.py:304-335); word_index [B,S] int32, -1 outside the word map;
 * word_key [B,S] int32 or NULL (= word_index), both as for mtvaf_span_propose.
 * A span (s, e) is valid iff 0 <= s <= e < S, word_index[s] >= 0 and word_index[e] >= 0.  Its signature is word_key[t]
 * wherever word_index[t] differs from the previous in-map token of the span (what mtvaf_span_propose de-duplicates by).
 * A predicted slot exists iff label_masks != 0, a gold slot iff gold_masks != 0.  The predicted class is the lowest k
 * whose logit no other logit exceeds (finite logits; NaN unspecified).  Every existing predicted slot adds 1 to
 * retrieved[class], valid or not; every existing gold slot adds 1 to relevant[gold_class], or to relevant_other when its
 * class is outside [0,K).  A valid predicted slot hits iff some valid gold slot of the sentence has an equal signature
 * and an equal class; a hit adds 1 to common[class], however many gold slots match.  An invalid slot of either side
 * never takes part in a match (an invalid gold slot is a term the feature truncated: eval_absa counts it in relevant).
 * counts [3K+2] int64: per class retrieved, relevant, common, then relevant_other, sentences (+B per call).  64-bit
 * integer atomics, one per block and non-zero counter: bit-reproducible.
 * pred_class [B,N] int32 or NULL: the class of every slot, -1 on a slot that does not exist; matched_gold [B,N] int32 or
 * NULL: the lowest matching gold slot, -1 without a hit.  Every element of a non-NULL output is written.
 * B >= 1, 1 <= S <= 512, 1 <= N <= 32, 1 <= G <= 32, 2 <= K <= 8 (MTVAF_ERR_SHAPE, checked before any launch). */
int mtvaf_span_counts(const int64_t* span_starts, const int64_t* span_ends, const int64_t* label_masks,
                      const float* logits, const int64_t* gold_starts, const int64_t* gold_ends,
                      const int64_t* gold_class, const int64_t* gold_masks, const int* word_index, const int* word_key,
                      int B, int S, int N, int G, int K, int64_t* counts, int* pred_class, int* matched_gold,
                      mtvaf_stream_t stream);

/* Tagger inference, the emitting half: the entities of decoded tags with the CRF posterior of each decoded segment.  It
 * complements the reference's decode (models/bert_model.py:511) and its host chunker (modules/eval_metrics.py::get_chunks).
 * One launch, no host read-back, no allocation, no workspace; safe under stream capture.
 * emissions [B,S,C] fp32; mask [B,S] u8, a PREFIX mask with mask[:,0] == 1 (ones, then zeros; L_b = the number of leading
 * ones; masks with holes are outside the contract: everything behind the first 0 is ignored).  tags [B,ldt] int32, ldt >= S,
 * as mtvaf_crf_viterbi writes them: only columns < L_b are read, an id outside [0,C) reads as 0.  keep [B,S] u8 names the
 * columns that take part in chunking (only columns < L_b count); NULL = columns 1 .. L_b-1.  start_tab / end_tab / type_of:
 * layout and meaning of mtvaf_entity_counts, index C = sentence boundary.  Over the kept labels l_j: a start at j iff
 * start_tab[l_j-1][l_j], an end at j iff end_tab[l_j][l_j+1]; every end with a start b <= j in the sentence closes one
 * chunk (type_of[l_j], b, j), b the greatest such start; an end without a start is dropped (neither emitted nor counted).
 * Per chunk, over ALL columns b..e (kept or not), each fixed to its decoded tag t_k:
 *   log_conf = alpha_b(t_b) + sum_{k=b+1..e} (trans[t_k-1][t_k] + em_k[t_k]) + beta_e(t_e) - logZ
 * with alpha / beta / logZ of the unconstrained chain over columns 0 .. L_b-1 (start and end included): the log posterior
 * of the decoded segment, <= 0 up to rounding, always finite (finite inputs).
 * ents [B,max_entities,3] int32 = (start column, end column, type), unused slots -1; log_conf [B,max_entities] fp32,
 * unused slots 0; count [B] int32 = chunks found, may exceed max_entities (then the first max_entities by end column are
 * stored).  Chunks are ordered by end column, ascending; every output element is written on every call.
 * 1 <= S <= 512, 1 <= C <= 64, ldt >= S (MTVAF_ERR_SHAPE); 1 <= n_types <= C+1, 1 <= max_entities <= 64 (MTVAF_ERR_ARG):
 * checked before any launch. */
int mtvaf_crf_entities(const float* emissions, const uint8_t* mask, const int32_t* tags, int ldt, const uint8_t* keep,
                       const float* start, const float* end, const float* trans, const uint8_t* start_tab,
                       const uint8_t* end_tab, const int* type_of, int n_types, int32_t* ents, float* log_conf,
                       int32_t* count, int B, int S, int C, int max_entities, mtvaf_stream_t stream);

/* Tagger inference: the posterior of every chunk EVENT -- for every span of kept columns and every type, the probability that
 * the chunker above (the reference's modules/eval_metrics.py::get_chunks on the tags of its decode, models/bert_model.py:511)
 * emits exactly that chunk -- under the chain over columns 0 .. L_b-1 restricted to the per-column tag sets of
 * mtvaf_crf_lattice_* (allowed int64 [B,S], 0 = the full set, bits >= C ignored; NULL = no constraint), start and end included.
 * One launch, no host read-back, no atomics, no allocation; safe under stream capture.
 * emissions, mask (a prefix mask; L_b = its leading ones), keep, start_tab / end_tab / type_of: as mtvaf_crf_entities reads them.
 * Kept columns k_0 < .. < k_n-1.  A non-kept column strictly between two kept columns must carry a singleton set; elsewhere
 * the kernel takes the LOWEST tag of its set there, for every quantity it computes (outside the contract).  Event (i, w, T),
 * b = k_i, e = k_i+w, 0 <= w < max_width, labels l_j of the kept columns with the boundary C on both sides:
 *   start_tab[l_i-1][l_i], no start_tab[l_j-1][l_j] for i < j <= i+w, end_tab[l_i+w][l_i+w+1], type_of[l_i+w] = T.
 * An end strictly inside the span does not exclude the event (the chunker emits both chunks then).
 * log_post [B,S,max_width,n_types] fp32, indexed by the start COLUMN b and the width w in kept columns: the log probability
 * of the event, -inf where it is impossible or undefined (b not kept, b >= L_b, the span runs past the last kept column).
 * logz_a [B] = log Z_A (0 for an empty sentence).  Every element of both is written on every call.
 * workspace: mtvaf_crf_chunk_posteriors_workspace_bytes(B, S, C) bytes (MTVAF_ERR_WORKSPACE if NULL or short).
 * 1 <= S <= 512, 1 <= C <= 64 (MTVAF_ERR_SHAPE); 1 <= n_types <= 64, 1 <= max_width <= 16 (MTVAF_ERR_ARG): checked before
 * the launch. */
size_t mtvaf_crf_chunk_posteriors_workspace_bytes(int B, int S, int C);
int mtvaf_crf_chunk_posteriors(const float* emissions, const int64_t* allowed, const uint8_t* mask, const uint8_t* keep,
                               const float* start, const float* end, const float* trans, const uint8_t* start_tab,
                               const uint8_t* end_tab, const int* type_of, int n_types, int max_width, float* log_post,
                               float* logz_a, int B, int S, int C, void* workspace, size_t workspace_bytes,
                               mtvaf_stream_t stream);

/* Calibration of entity posteriors, the counting half: per entity type and log-probability bin, how many scored items there
 * are, how many of them are gold chunks, sum p and sum (p - y)^2, ADDED into a device counter block.  Two launches on the
 * stream (one block per sentence, then one block that sums the sentences in order); no host read-back, no allocation, no
 * atomics on global memory and no floating-point atomics: safe under stream capture, and the same inputs give the same bits.
 * gold [B,S] int64 labels, an id outside [0,C) reads as 0; mask [B,S] u8, a prefix mask (L_b = its leading ones); keep
 * [B,S] u8 or NULL (= columns 1 .. L_b-1; only columns < L_b count); start_tab / end_tab / type_of / n_types exactly as
 * mtvaf_crf_entities reads them.  The gold chunks of a sentence are the chunks mtvaf_crf_entities' chunker emits on the
 * gold labels of the kept columns: every end with a start b <= j closes (type, b, j), b the greatest such start; an end
 * without a start is dropped.
 * edges [n_bins+1] fp32, ascending log-probability bin edges.  The bin of lp is the number of k in 1 .. n_bins-1 with
 * lp >= edges[k], compared on the stored fp32 values: no exponential decides a bin, so a host that compares the same array
 * agrees exactly.  edges[0] and edges[n_bins] are not read for binning.
 * counter: 4*T*NB + 2*T + 1 words of 8 bytes (T = n_types, NB = n_bins), in this order:
 *   n[T][NB] int64 scored items; hit[T][NB] int64 scored items that are a gold chunk; gold[T] int64 gold chunks;
 *   gold_reachable[T] int64 gold chunks no wider than max_width kept columns (chunk form; = gold in the entity form);
 *   sum_p[T][NB] double, sum of p = exp((double)lp); sum_sq[T][NB] double, sum of (p - y)^2, y = 1 on a hit, else 0;
 *   sentences int64, + B per call.
 * The double sums are reduced in a fixed order: within a wave in ascending lane order, the block's waves in wave order, the
 * sentences in sentence order.  workspace: mtvaf_calibration_workspace_bytes(B, n_types, n_bins) bytes (0 for arguments out
 * of range), MTVAF_ERR_WORKSPACE if NULL or short; it need not be cleared.
 * mtvaf_chunk_calibration scores dense events: log_post [B,S,max_width,n_types] fp32 as mtvaf_crf_chunk_posteriors writes
 * it (start column b, width w in kept columns, type).  Every element with lp > -inf is one scored item of its type; -inf
 * and NaN elements are skipped and not counted.  It is a hit iff a gold chunk of that type starts at column b and ends at
 * the kept column w places after b's ordinal among the kept columns.
 * mtvaf_entity_calibration scores listed entities: ents [B,max_entities,3] int32 (start column, end column, type; -1 in
 * an unused slot) and log_conf [B,max_entities] fp32, the format of mtvaf_crf_entities.  A slot whose type is outside
 * [0,n_types) or whose columns are outside [0,S) is skipped (so is an unused one); every other slot is one scored item, a
 * hit iff a gold chunk has the same start column, end column and type; a slot whose log_conf is -inf or NaN is counted in
 * bin 0 with p = 0.  A slot listed twice counts twice.
 * B >= 1, 1 <= S <= 512, 1 <= C <= 64 (MTVAF_ERR_SHAPE); 1 <= n_types <= 64, 1 <= max_width <= 16, 1 <= max_entities <= 64,
 * 1 <= n_bins <= 64 (MTVAF_ERR_ARG): checked before any launch. */
size_t mtvaf_calibration_workspace_bytes(int B, int n_types, int n_bins);
int mtvaf_chunk_calibration(const float* log_post, const int64_t* gold, const uint8_t* mask, const uint8_t* keep,
                            const uint8_t* start_tab, const uint8_t* end_tab, const int* type_of, const float* edges, int B,
                            int S, int C, int n_types, int max_width, int n_bins, void* counter, void* workspace,
                            size_t workspace_bytes, mtvaf_stream_t stream);
int mtvaf_entity_calibration(const int32_t* ents, const float* log_conf, const int64_t* gold, const uint8_t* mask,
                             const uint8_t* keep, const uint8_t* start_tab, const uint8_t* end_tab, const int* type_of,
                             const float* edges, int B, int S, int C, int n_types, int max_entities, int n_bins, void* counter,
                             void* workspace, size_t workspace_bytes, mtvaf_stream_t stream);

/* Cutoff augmentation on the embedding output (modules/augument.py:99-159): out = x * row_keep[b,s] * col_keep[b,:]
 * (either mask may be NULL); x/out [B,S,H] fp32, row_keep [B*S], col_keep [B,H].  Self-adjoint: the backward is the
 * same call on the gradient. */
int mtvaf_mask_mul(const float* x, const float* row_keep, const float* col_keep, float* out, int B, int S, int H,
                   mtvaf_stream_t stream);

/* bf16-OPERAND GEMM of the mixed-precision mode (new functionality: the reference has no mixed precision, SURVEY.md
 * fact 8): C[M,N] = opA[M,K] . opB[K,N] with A, B stored as bf16 and fp32 accumulation.  layout 0 (KC): reduction index
 * contiguous (A[m][k], B[n][k]); layout 1 (KM): reduction index is the row (A[k][m], B[k][n]) -- so the forward product
 * (0,0), dX = dY.W (0,1) and dW = dY^T.X (1,1) all read the same row-major bf16 tensors (transposing LDS reads; no
 * transposed copies).  Results: C32 fp32 and / or C16 bf16 (either may be NULL); accumulate adds into C32.  epi 0 none,
 * 1 bias + erf-GELU (pre-activation saved to aux16 as bf16), 3 multiply by GELU'(aux16).  colpart [M/128][N] (optional):
 * per-tile column sums of the result, finished by mtvaf_colsum_small (the bias gradient of the layer that produced the
 * operand).  Deterministic split-K as mtvaf_gemm_f32 (fp32 result only).  Aligned shapes only (M % 128, N % 128 or N % 96, K % 64, ld % 8, 16-byte aligned pointers): MTVAF_ERR_SHAPE / _ALIGN otherwise.
 * tile: 0 auto, 1 128x96, 2 128x128, 3 256x128 (8 waves; layout_a 0, M % 256 == 0, no colpart), 4 256x192 (8 waves;
 * layout_a 0, M % 256 == 0, N % 192 == 0); stages: 0 auto, 2 (two blocks per CU), 3..5 (one block, stages - 1 k-tiles
 * in flight; the 256x192 tile always runs its 2-stage ring).
 * mtvaf_cast_bf16 makes the bf16 copies of the fp32 master weights. */
int mtvaf_gemm_bf16x(int layout_a, int layout_b, const void* A, int lda, const void* B, int ldb, float* C32, int ldc32,
                     void* C16, int ldc16, int M, int N, int K, const float* bias, int epi, void* aux16, int ldaux,
                     int accumulate, float* colpart, int allow_split, void* workspace, size_t workspace_bytes, int tile,
                     int splits, int stages, mtvaf_stream_t stream);
/* ... for a weight-gradient product (KM x KM) whose operand A is exactly zero outside the listed 64-row k-tiles of the token
 * axis (mtvaf_build_ktiles with bk = 64): see mtvaf_gemm_f32_ktiles. */
int mtvaf_gemm_bf16x_ktiles(int layout_a, int layout_b, const void* A, int lda, const void* B, int ldb, float* C32, int ldc32,
                            void* C16, int ldc16, int M, int N, int K, const float* bias, int epi, void* aux16, int ldaux,
                            int accumulate, float* colpart, int allow_split, void* workspace, size_t workspace_bytes, int tile,
                            int splits, int stages, const int* klist, const int* kcnt, mtvaf_stream_t stream);
int mtvaf_colsum_small(const float* part, int rows, int cols, float* out, int accumulate, mtvaf_stream_t stream);
/* mtvaf_gemm_f32 computed on the bf16 matrix pipe: each fp32 operand value is split into three bf16 planes while its tile
 * is staged into the LDS and a product is the six significant bf16 MFMA products, accumulated in fp32 (the dropped terms are
 * below 2^-26 |a||b|: accuracy of the fp32 pipe; operands and results stay fp32 in memory).  Same arguments as
 * mtvaf_gemm_f32 (modeling_bert.py:266, 283-284, 353, 420-421, 433 and their autograd backward); shapes it does not cover
 * (not whole 64x64 tiles, K % 32 != 0, unaligned operands) run the fp32 pipe.  mtvaf_f32_split(1 / 0): mtvaf_gemm_f32 and
 * mtvaf_gemm_f32_ktiles use it everywhere they can / never (default: 1; MTVAF_F32_SPLIT=0 in the environment: 0); -1 queries.
 * Domain: operands at or above 2^127 (2 - 2^-8) ~ 3.396e38 in magnitude round to an infinite first plane and give non-finite
 * results on the split arithmetic (here and from plane images), while the fp32 pipe stays finite; inf and NaN operands give
 * non-finite results on both. */
int mtvaf_gemm_f32x3(int layout_a, int layout_b, const float* A, int lda, const float* B, int ldb, float* C, int ldc,
                     int M, int N, int K, const float* bias, int epi, float* aux, int ldaux, int accumulate,
                     int allow_split, void* workspace, size_t workspace_bytes, int cfg, int splits,
                     mtvaf_stream_t stream);
int mtvaf_f32_split(int on);
/* profiling hook (tools/x3_trace.py): block 0 of every following wave-specialised split launch stores per wave and k-tile the
 * shader clock around the tile barrier into buf ([8 waves][64 k-tiles][4] + 17 int64 on the device); NULL switches it off */
/* Round 5: a dense product in front of a LayerNorm may leave its split-K slabs unreduced -- the LayerNorm adds them itself, in
 * the order the reduction launch would (modeling_bert.py:353-355, 433-435 and their autograd backward).  mtvaf_gemm_f32_slabs =
 * mtvaf_gemm_f32 with a plain epilogue: *splits_out == 1: C holds the result (+ bias, accumulate); s > 1: `workspace` holds s slabs
 * [M][N] (slab stride M * N floats), neither bias nor accumulate applied, C untouched.  mtvaf_dropout_res_ln_fwd_slabs: x = slab 0
 * + ... + bias is stored to x_out (the backward pass reads it), then as mtvaf_dropout_res_ln_fwd.  mtvaf_dropout_res_ln_bwd_rows_slabs:
 * dout = (slab 0 + ...) + dout_base, then as mtvaf_dropout_res_ln_bwd_rows. */
int mtvaf_gemm_f32_slabs(int layout_a, int layout_b, const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N,
                         int K, const float* bias, int accumulate, void* workspace, size_t workspace_bytes, int* splits_out,
                         mtvaf_stream_t stream);
int mtvaf_dropout_res_ln_fwd_slabs(const float* slabs, int nslab, const float* bias, float* x_out, const float* res, const float* gamma,
                                   const float* beta, float* out, float* mean, float* rstd, int M, int H, float eps, double p_drop,
                                   uint64_t seed, uint64_t offset, void* out_bf16, mtvaf_stream_t st);
int mtvaf_dropout_res_ln_bwd_rows_slabs(const float* dout_base, const float* slabs, int nslab, const float* x, const float* res,
                                        const float* gamma, const float* mean, const float* rstd, float* dx, float* dres,
                                        int dres_accumulate, int M, int H, double p_drop, uint64_t seed, uint64_t offset, float* part,
                                        void* dx_bf16, mtvaf_stream_t st);
/* Round 5, pre-split operands: the two LayerNorm kernels that ALSO write the tile-blocked plane image [H / 32][3][M][32] of their
 * output (H % 32 == 0), bit for bit what mtvaf_f32_split_planes would write behind them.  _fwd_planes: nslab == 0 -> x is the dense
 * output (as mtvaf_dropout_res_ln_fwd), nslab >= 1 -> x = the product's unreduced slabs (as mtvaf_dropout_res_ln_fwd_slabs).
 * _bwd_rows_planes: nslab == 0 -> dout = dout_base (as mtvaf_dropout_res_ln_bwd_rows), nslab >= 1 -> dout = slabs + dout_base; dx may
 * be NULL (a gradient only GEMMs read). */
int mtvaf_dropout_res_ln_fwd_planes(const float* x, int nslab, const float* bias, float* x_out, const float* res, const float* gamma,
                                    const float* beta, float* out, float* mean, float* rstd, int M, int H, float eps, double p_drop,
                                    uint64_t seed, uint64_t offset, void* out_planes, mtvaf_stream_t st);
int mtvaf_dropout_res_ln_bwd_rows_planes(const float* dout_base, const float* slabs, int nslab, const float* x, const float* res,
                                         const float* gamma, const float* mean, const float* rstd, float* dx, float* dres,
                                         int dres_accumulate, int M, int H, double p_drop, uint64_t seed, uint64_t offset, float* part,
                                         void* dx_planes, mtvaf_stream_t st);
int mtvaf_f32x3_trace(void* buf);

/* Pre-split operands (csrc/gemm_f32p.hip, round 5; the same nn.Linear products, modeling_bert.py:266, 283-284, 353, 420-421,
 * 433).  mtvaf_f32_split_planes writes the three bf16 planes x = x1 + x2 + x3 of an fp32 matrix [rows][cols] (the split of
 * csrc/gemm_f32x3.hip, bit for bit) as a plane image addressed by three BYTE strides: plane -> plane, row -> row, 32-column
 * k-tile -> k-tile (natural form: cols * 2 * rows / ld * 2 / 64; tile-blocked form [k-tile][plane][rows][32]: rows * 64 / 64 /
 * 3 * rows * 64).  An element at or above 2^127 (2 - 2^-8) in magnitude has an infinite first plane (RNE to bf16 overflows), then an
 * infinite and a NaN plane: operands from there on give non-finite results on the split arithmetic, while the fp32 pipe stays finite.
 * mtvaf_gemm_f32p: C[M,N] = A[M,K] . op(B) (+ bias, epilogue, accumulate) from the plane images of both
 * operands on v_mfma_f32_16x16x32_bf16, nothing split inside the k-loop; layout_b 0: B [N][K] (forward), 1: B [K][N] (the dX
 * products: natural plane image, b_row = N * 2, b_kt = 32 * N * 2, b_col = 256); layout_a 1 (with layout_b 1): A [K][M] too, the
 * weight-gradient products; M, N % 128 == 0, K % 32 == 0; splits > 1 = deterministic
 * split-K through `workspace`; ablate = 0 (research switches: 1 no MFMAs, 2 no requests, 4 no fragment reads: timing only).
 * mtvaf_f32p_trace: shader-clock stamps of block 0 ([8 waves][64 k-tiles][2] + 17 int64), NULL = off. */
int mtvaf_f32_split_planes(const float* src, void* dst, int rows, int cols, int ld, long s_plane, long s_row, long s_kt,
                           mtvaf_stream_t stream);
int mtvaf_gemm_f32p(int layout_a, const void* Aplanes, long a_plane, long a_row, long a_kt, long a_col, int layout_b, const void* Bplanes,
                    long b_plane, long b_row, long b_kt, long b_col, float* C, int ldc, int M, int N, int K, const float* bias, int epi,
                    float* aux, int ldaux, int accumulate, int splits, void* workspace, size_t workspace_bytes, int ablate,
                    mtvaf_stream_t stream);
int mtvaf_f32p_trace(void* buf);
/* The tile of mtvaf_gemm_f32p* (round 6): which products may run on the 128 x 256 tile (csrc/gemm_f32pw.hip; N % 256 == 0) instead of
 * the 128 x 128 tile -- a mask: 1 = forward products (layout_b 0; these may also take a 128 x 192 tile when N % 192 == 0 and no
 * plane-image result is asked for), 2 = dX products (layout_b 1), 4 = weight gradients (layout_a 1; the grouped launch when every
 * N_i % 256 == 0).  Among the admitted tiles a launch takes the cheapest by an estimate of rounds x tile time (QKV forward at 2432
 * rows: 192 columns, one round of 228 tiles; FFN-1: 256; N = 768 and 4096-row launches: mostly 128 x 128).  8 = never the 128 x 128
 * tile where another can serve (tests), 16 = never the 128 x 192 tile.  mask >= 0 sets, -1 queries; returns the mask in force
 * (default 7).  Process-global; placement only -- the kernels issue the same MFMA products in the same
 * order for every output element and agree bit for bit. */
int mtvaf_f32p_wide(int mask);
/* research entry: up to four weight-gradient products C_i [M_i][N_i] = A_i^T . B_i from plane images (A_i [K][M_i], B_i [K][N_i], the
 * token rows K shared) in ONE unsplit launch over the 128 x 128 tiles of all of them -- what the grouped launch of
 * mtvaf_gemm_f32_dw_group becomes with pre-split operands (no bias sums, no k-tile list).  strides: eight byte strides per product
 * (a_plane, a_row, a_kt, a_col, b_plane, b_row, b_kt, b_col; natural image of [K][C]: C*K*2, C*2, 64*C, 256; tile-blocked image
 * [C/32][3][K][32]: K*64, 64, 2048, 12*K*64).  M_i, N_i % 128 == 0, K % 32 == 0. */
int mtvaf_gemm_f32p_dw_group(int n, const void* const* Aplanes, const void* const* Bplanes, const long* strides, float* const* C, const int* ldc,
                             const int* M, const int* N, int K, mtvaf_stream_t stream);
/* ... with up to eight column-sum jobs as extra blocks of the same launch: job j sums the fp32 matrix cs_src[j] [cs_rows[j]][cs_cols[j]]
 * (leading dimension cs_ld[j]) over its rows into cs_dst[j]; fixed summation order.  The small reductions of a layer's backward pass
 * (QKV / FFN-1 bias gradients, the two LayerNorm-backward finishes) ride in the CUs the last round of tiles leaves idle. */
int mtvaf_gemm_f32p_dw_group_colsum(int n, const void* const* Aplanes, const void* const* Bplanes, const long* strides, float* const* C,
                                    const int* ldc, const int* M, const int* N, int K, int njobs, const float* const* cs_src,
                                    const int* cs_rows, const int* cs_cols, const int* cs_ld, float* const* cs_dst, mtvaf_stream_t stream);
/* The two entries above with an `accumulate` flag (njobs 0 .. 8): != 0 -> every tile stores old + product and every column-sum job
 * old + sum.  Product and sum are formed exactly as by the overwriting form and the destination's old value is added once, last, so
 * the result is one IEEE add away from it (gradient accumulation over micro-batches).  0: those entries, bit for bit. */
int mtvaf_gemm_f32p_dw_group_acc(int n, const void* const* Aplanes, const void* const* Bplanes, const long* strides, float* const* C,
                                 const int* ldc, const int* M, const int* N, int K, int njobs, const float* const* cs_src,
                                 const int* cs_rows, const int* cs_cols, const int* cs_ld, float* const* cs_dst, int accumulate,
                                 mtvaf_stream_t stream);
/* mtvaf_gemm_f32p with a plain epilogue that leaves a split-K plan's slabs unreduced (as mtvaf_gemm_f32_slabs: *splits_out = 1 -> C
 * holds the result; s > 1 -> `workspace` holds s slabs [M][N], bias / accumulate not applied): the LayerNorm kernels behind the Wo /
 * FFN-2 / FFN-1 dX products add them (modeling_bert.py:353-355, 433-435 and their backward). */
int mtvaf_gemm_f32p_slabs(int layout_a, const void* Aplanes, long a_plane, long a_row, long a_kt, long a_col, int layout_b, const void* Bplanes,
                          long b_plane, long b_row, long b_kt, long b_col, float* C, int ldc, int M, int N, int K, const float* bias,
                          int accumulate, int splits, void* workspace, size_t workspace_bytes, int* splits_out, mtvaf_stream_t stream);
/* mtvaf_gemm_f32p, unsplit, whose result is written as a tile-blocked plane image c_planes [N / 32][3][M][32] -- beside the fp32
 * result (C != NULL) or instead of it (C == NULL: a tensor that only GEMMs read: the GELU output between the two FFN products, the
 * GELU' output between their dX products) -- and, optionally, its per-tile column sums colpart [M / 128][N] (finished by
 * mtvaf_colsum_small: the FFN-1 bias gradient). */
int mtvaf_gemm_f32p_ep(int layout_a, const void* Aplanes, long a_plane, long a_row, long a_kt, long a_col, int layout_b, const void* Bplanes,
                       long b_plane, long b_row, long b_kt, long b_col, float* C, int ldc, void* c_planes, float* colpart, int M, int N, int K,
                       const float* bias, int epi, float* aux, int ldaux, int accumulate, mtvaf_stream_t stream);

/* The (up to four) weight-gradient products of one encoder layer in fp32, dW_i[M_i,N_i] = A_i^T . B_i with A_i [K,M_i], B_i [K,N_i]
 * row-major, as ONE launch of the 128x96 LDS-DMA kernel (autograd backward of modeling_bert.py:266, 283-284, 353, 420-421, 433);
 * klist / kcnt as mtvaf_gemm_f32_ktiles (NULL: the whole reduction); deterministic split-K through per-product slabs in
 * `workspace` (splits <= 0: planned).  M_i % 128 == 0, N_i % 96 == 0, K % 32 == 0.  Under the split arithmetic (mtvaf_f32_split),
 * for K > 1024 and M_i, N_i % 128 == 0, the launch is the GROUP form of the wave-specialised split kernel on 128x128 tiles
 * instead (unsplit once the tiles cover three quarters of the CUs: 432 tiles at BERT-base).  mtvaf_dw_group_rows: the executor
 * groups layers of at most that many token rows on the fp32 pipe's ring (default 1024, MTVAF_DW_GROUP_ROWS; rows >= 0 sets,
 * -1 queries); mtvaf_dw_group_wanted(rows, H, I): the executor's whole rule (1: this layer's weight gradients go out grouped). */
int mtvaf_gemm_f32_dw_group(int n, const float* const* A, const int* lda, const float* const* B, const int* ldb, float* const* C,
                            const int* ldc, const int* M, const int* N, int K, const int* klist, const int* kcnt,
                            void* workspace, size_t workspace_bytes, int splits, mtvaf_stream_t stream);
/* bytes of split-K slabs that call needs for these products (0: no split planned; too little workspace is MTVAF_ERR_WORKSPACE,
 * never a silently different plan) */
size_t mtvaf_gemm_f32_dw_group_workspace_bytes(int n, const int* M, const int* N, int K, int splits);
/* The same launch + the bias gradients that go with the weight gradients: dbias (nullable array of n nullable pointers),
 * dbias[i][0 .. M_i) <- column sums of A_i over its K rows (A_i is the dY of the dense layer: autograd backward of the bias of
 * modeling_bert.py:266, 283-284, 420-421), 16-byte aligned, overwritten.  The unsplit grouped launch of the split kernel
 * takes them from the A tiles it stages anyway; any other plan runs mtvaf_colsum behind the products (workspace_bytes must
 * then also cover mtvaf_colsum_workspace_bytes(K, M_i)). */
int mtvaf_gemm_f32_dw_group_bias(int n, const float* const* A, const int* lda, const float* const* B, const int* ldb,
                                 float* const* C, const int* ldc, const int* M, const int* N, int K, const int* klist,
                                 const int* kcnt, float* const* dbias, void* workspace, size_t workspace_bytes, int splits,
                                 mtvaf_stream_t stream);
/* mtvaf_gemm_f32_dw_group_bias (dbias nullable) with an `accumulate` flag: != 0 -> dW_i += the product, dbias_i += the column sums,
 * each one add behind the value the overwriting form stores (the same plan on the same kernels: the old value enters in the
 * epilogue of an unsplit launch, in the ordered slab reduction of a split one).  0: that entry, bit for bit. */
int mtvaf_gemm_f32_dw_group_acc(int n, const float* const* A, const int* lda, const float* const* B, const int* ldb,
                                float* const* C, const int* ldc, const int* M, const int* N, int K, const int* klist,
                                const int* kcnt, float* const* dbias, void* workspace, size_t workspace_bytes, int splits,
                                int accumulate, mtvaf_stream_t stream);
int mtvaf_dw_group_rows(int rows);
int mtvaf_dw_group_wanted(int rows, int H, int I);

/* Stream-K form of the 256x256 eight-phase bf16 kernel (csrc/gemm_bf16p.hip; tile 5 = tile-per-block, tile 6 = stream-K forced,
 * tile 0 = the planner decides): one block per CU walks an equal run of the k-tile steps of all output tiles; a tile whose
 * reduction is shared by several blocks is combined inside the launch (fp32 contributions in block order = k order, published
 * with an agent-scope release and consumed behind an agent-scope acquire: deterministic for a given scratch size).  The
 * contributions live in a caller-owned scratch attached per stream: at least mtvaf_streamk_scratch_bytes(256) bytes, 16-byte
 * aligned, zero-initialised by the caller, alive until replaced or detached (scratch = NULL).  Replaces nothing in the
 * reference (new functionality of the mixed-precision mode); the products are those of modeling_bert.py:266, 283-284, 353,
 * 420-421, 433 and their autograd backward. */
int mtvaf_streamk_attach(void* scratch, size_t bytes, mtvaf_stream_t stream);
size_t mtvaf_streamk_scratch_bytes(int blocks);
int mtvaf_streamk_attached(mtvaf_stream_t stream); /* -> blocks the attached scratch serves, 0: none */
/* The (up to four) weight-gradient products of one encoder layer, dW_i[M_i,N_i] = A_i^T . B_i with A_i [K,M_i], B_i [K,N_i] bf16
 * row-major and fp32 results, in ONE stream-K launch (autograd backward of modeling_bert.py:266, 283-284, 353, 420-421, 433).
 * Needs an attached scratch (MTVAF_ERR_WORKSPACE otherwise); M_i % 256 == 0, N_i % 256 == 0, K % 64 == 0. */
int mtvaf_gemm_bf16x_dw_group(int n, const void* const* A, const int* lda, const void* const* B, const int* ldb, float* const* C32,
                              const int* ldc32, const int* M, const int* N, int K, mtvaf_stream_t stream);
/* ... with an `accumulate` flag: != 0 -> C32_i += the product: the block that finishes a tile adds the old value behind the
 * contributions it has combined in k order; a block that only contributes never reads the destination.  0: the entry above. */
int mtvaf_gemm_bf16x_dw_group_acc(int n, const void* const* A, const int* lda, const void* const* B, const int* ldb, float* const* C32,
                                  const int* ldc32, const int* M, const int* N, int K, int accumulate, mtvaf_stream_t stream);
/* The cut mtvaf_gemm_bf16x_dw_group[_acc] takes for these products on `stream`: the pieces S every tile's reduction is divided into (1: whole tiles, no
 * block contributes to another's tile; S > 1: S - 1 contributing blocks and one finishing block per tile).  0: the call would be
 * refused (shapes, or no scratch attached to the stream).  The launch's own planner call. */
int mtvaf_gemm_bf16x_dw_group_pieces(int n, const int* M, const int* N, int K, mtvaf_stream_t stream);

/* Prefix attention of the mixed-precision mode: the algorithm of mtvaf_prefix_attn_fwd / _bwd (same key order, mask,
 * dropout hash) on bf16 operands with fp32 softmax statistics and accumulation.  qkv16 [B*S,3H], pk16 / pv16 [B,P*H],
 * ctx16 [B*S,H], dctx16, dqkv16: bf16; lse [B,NH,S], dpk / dpv [B,P*H]: fp32.  The backward also emits per-block column
 * sums partq [B*ceil(S/64)][H] (dQ) and partkv [B*ceil((P+S)/64)][2H] (dK | dV over the text keys): summed over their rows
 * (mtvaf_colsum_small / mtvaf_colsum) they are the query / key / value bias gradients. */
int mtvaf_prefix_attn_bf16_fwd(const void* qkv16, const void* pk16, const void* pv16, const float* addmask, void* ctx16,
                               float* lse, int B, int S, int P, int NH, int head_dim, float p_drop, uint64_t seed,
                               uint64_t offset, mtvaf_stream_t stream);
int mtvaf_prefix_attn_bf16_bwd(const void* dctx16, const void* qkv16, const void* pk16, const void* pv16,
                               const float* addmask, const void* ctx16, const float* lse, void* dqkv16, float* dpk,
                               float* dpv, float* partq, float* partkv, int B, int S, int P, int NH, int head_dim,
                               float p_drop, uint64_t seed, uint64_t offset, mtvaf_stream_t stream);
/* mtvaf_prefix_attn_bf16_bwd under the zero-tail contract of mtvaf_prefix_attn_bwd_tail (the key side's query loop stops at the
 * last unmasked position; same bits) */
int mtvaf_prefix_attn_bf16_bwd_tail(const void* dctx16, const void* qkv16, const void* pk16, const void* pv16,
                                    const float* addmask, const void* ctx16, const float* lse, void* dqkv16, float* dpk,
                                    float* dpv, float* partq, float* partkv, int B, int S, int P, int NH, int head_dim,
                                    float p_drop, uint64_t seed, uint64_t offset, int zero_tail, mtvaf_stream_t stream);
/* ... over PACKED token rows (padding-free execution, see mtvaf_prefix_attn_varlen_fwd): cu [B+1] int32, no mask read;
 * partq / partkv keep their padded row counts (blocks beyond a sentence write zeros). */
int mtvaf_prefix_attn_bf16_varlen_fwd(const void* qkv16, const void* pk16, const void* pv16, const int* cu, int pad_rows, void* ctx16,
                                      float* lse, int B, int S, int P, int NH, int head_dim, float p_drop, uint64_t seed,
                                      uint64_t offset, mtvaf_stream_t stream);
int mtvaf_prefix_attn_bf16_varlen_bwd(const void* dctx16, const void* qkv16, const void* pk16, const void* pv16, const int* cu,
                                      int pad_rows, const void* ctx16, const float* lse, void* dqkv16, float* dpk, float* dpv, float* partq,
                                      float* partkv, int B, int S, int P, int NH, int head_dim, float p_drop, uint64_t seed,
                                      uint64_t offset, mtvaf_stream_t stream);
/* ... with a per-sentence prefix-slot mask (see mtvaf_prefix_attn_varlen_fwd_pm): pmask [B, P] fp32 additive, pmask_len = B * P;
 * pmask == NULL: the launch of mtvaf_prefix_attn_bf16_varlen_fwd / _bwd. */
int mtvaf_prefix_attn_bf16_varlen_fwd_pm(const void* qkv16, const void* pk16, const void* pv16, const int* cu, int pad_rows,
                                         const float* pmask, long pmask_len, void* ctx16, float* lse, int B, int S, int P, int NH,
                                         int head_dim, float p_drop, uint64_t seed, uint64_t offset, mtvaf_stream_t stream);
int mtvaf_prefix_attn_bf16_varlen_bwd_pm(const void* dctx16, const void* qkv16, const void* pk16, const void* pv16, const int* cu,
                                         int pad_rows, const float* pmask, long pmask_len, const void* ctx16, const float* lse,
                                         void* dqkv16, float* dpk, float* dpv, float* partq, float* partkv, int B, int S, int P, int NH,
                                         int head_dim, float p_drop, uint64_t seed, uint64_t offset, mtvaf_stream_t stream);
int mtvaf_cast_bf16(const float* x, int ldx, void* out, int ldo, void* outT, int ldt, int R, int C,
                    mtvaf_stream_t stream);

/* ---- native per-layer executor ----------------------------------------------------------
 * One call enqueues ALL kernels of a BertLayer forward / backward (models/modeling_bert.py:439-522 and its autograd
 * backward) -- the same kernels in the same order as the Python engine, composed inside the library -- so a training step
 * costs one host call per layer and direction instead of ~65.  `bf16` selects the kernel family: 0 = fp32 (qkv / cx / pre /
 * act are float*, weights w*, prefix slabs float*), 1 = mixed precision (those four are bf16, weights the bf16 images
 * w*_h, x_h / h1_h / h2_h bf16 copies, prefix slabs bf16).  Dropout sites: attention `offset`, attention output
 * `offset + 1`, FFN output `offset + 2`.  All buffers caller-owned; workspaces as the composed entry points need them. */
typedef struct {
  int B, S, P, NH, H, I;
  int bf16;
  float eps;
  double p_hidden; /* a double: the LayerNorm sites scale kept elements by float(1 / (1 - p)), as torch does */
  float p_attn;
  uint64_t seed, offset;
  const float *wqkv, *wo, *w1, *w2;        /* fp32 masters [3H,H] [H,H] [I,H] [H,I] (fp32 mode) */
  const void *wqkv_h, *wo_h, *w1_h, *w2_h; /* bf16 images (bf16 mode) */
  const float *bqkv, *bo, *g1, *b1, *bi1, *bi2, *g2, *b2;
  const float* x;                          /* [M,H] layer input */
  const void* x_h;                         /* bf16 copy (bf16 mode) */
  const void *pk, *pv;                     /* prefix slabs [B, P*H] or NULL */
  const float* addmask;                    /* [B, P+S] */
  void *qkv, *cx;                          /* [M,3H], [M,H] */
  float *lse, *a, *h1;                     /* [B,NH,S], [M,H], [M,H] */
  void* h1_h;
  float *mean1, *rstd1;
  void *pre, *act;                         /* [M,I] */
  float *f, *h2;                           /* [M,H] */
  void* h2_h;
  float *mean2, *rstd2;
  void* ws; size_t ws_bytes;               /* main-stream scratch of the forward pass (split-K slabs of small-M products) */
  /* padding-free execution: cu != NULL -> the token tensors (x, qkv ... h2, and the gradient buffers) hold Mp
   * PACKED rows -- the Mv unmasked tokens sentence by sentence (cu [B+1] int32 row offsets), then Mp - Mv zero rows that
   * pad the image to whole 128-row tiles; lse / delta keep [B,NH,S].  cu == NULL: the padded [B*S] layout. */
  const int* cu;
  int Mv, Mp;
  /* fp32 mode, optional (round 5; all of them, with the weights' plane images in w*_h, packed rows, H and I % 128 == 0): PRE-SPLIT
   * operands -- tile-blocked plane images ([cols / 32][3][Mp][32] bf16: mtvaf_f32_split_planes with strides Mp * 64 / 64 / 3 * Mp * 64) of
   * the layer input x_p (given), and of the attention context, the attention-block output, the GELU output and the layer output
   * (written here: cx_p, h1_p, act_p, h2_p = the next layer's x_p, or NULL).  The eight forward / dX products and the grouped weight
   * gradients then run on the pre-split kernels of csrc/gemm_f32p.hip (nothing split inside their k-loops). */
  const void* x_p;
  void *cx_p, *h1_p, *act_p, *h2_p;
  /* packed rows, optional: the per-sentence prefix-slot mask [B, P] (mtvaf_prefix_attn_varlen_fwd_pm; the prefix columns of
   * addmask, which packed rows do not read) or NULL -- every sentence owns all P slots.  Ignored in the padded layout. */
  const float* pmask;
} mtvaf_layer_t;

typedef struct {
  float* dh;                              /* in: d loss / d h2 [M,H]; out: d loss / d x */
  float* dh1;                             /* [M,H] scratch */
  void *df, *dpre, *da, *dctx, *dqkv;     /* [M,H] [M,I] [M,H] [M,H] [M,3H]  (bf16 in bf16 mode) */
  float *part, *partq, *partkv;           /* bf16 mode: epilogue / attention column-sum partials
                                           * [M/128, I], [B*ceil(S/64), H], [B*ceil((P+S)/64), 2H] */
  float* delta;                           /* fp32 mode: [B,NH,S] */
  float *dwqkv, *dbqkv, *dwo, *dbo, *dg1, *db1, *dw1, *dbi1, *dw2, *dbi2, *dg2, *db2;
  float *dpk, *dpv;                       /* [B, P*H] or NULL */
  void* ws_main; size_t ws_main_bytes;    /* scratch of the main stream (LayerNorm partials, split-K slabs) */
  void* ws_side; size_t ws_side_bytes;    /* scratch of the second stream (split-K slabs, column-sum partials) */
  /* optional: k-tile list of the token axis for the weight-gradient products (mtvaf_build_ktiles; 32-row tiles in fp32
   * mode, 64-row tiles in bf16 mode) */
  const int* klist;
  const int* kcnt;
  /* the caller's word: token rows behind a sentence's last unmasked position carry exactly-zero gradients (what a k-tile list
   * implies as well): the attention backward stops its query loops there (mtvaf_prefix_attn_bwd_tail) */
  int zero_tail;
  /* optional (both or neither; required with plane images): the layer's own LayerNorm-backward partials of the FFN / attention
   * block, mtvaf_ln_bwd_workspace_bytes(M, H) each -- their column sums then run on `side` instead of the main chain */
  float *lnpart2, *lnpart1;
  /* fp32 mode with pre-split operands (see mtvaf_layer_t::x_p): scratch plane images of the four upstream gradients that are GEMM
   * operands -- [Mp, H], [Mp, I], [Mp, H], [Mp, 3H] -- alive until the second stream has finished the layer's weight gradients;
   * with `part`, both lnpart and ws_main they are required when the layer struct has plane images, NULL otherwise */
  void *df_p, *dpre_p, *da_p, *dqkv_p;
  /* != 0: the sixteen parameter gradients (dwqkv .. db2) are ADDED to: every launch that writes one takes its accumulating form
   * (value formed as at 0, the old value added once, last).  dh, dpk and dpv are activations' gradients and are always overwritten.
   * 0: every launch is what it was before this field existed. */
  int accumulate;
} mtvaf_layer_grads_t;

int mtvaf_encoder_layer_fwd(const mtvaf_layer_t* layer, mtvaf_stream_t stream);
/* weight-gradient products on `side` behind events of `main` (side == main serialises); settle != 0: `side` also waits for
 * the layer's last main-stream kernel (an optimizer update hanging off the caller's hook must not overtake it). */
int mtvaf_encoder_layer_bwd(const mtvaf_layer_t* layer, const mtvaf_layer_grads_t* grads, mtvaf_stream_t main,
                            mtvaf_stream_t side, int settle);
size_t mtvaf_layer_struct_bytes(int which /* 0: mtvaf_layer_t, 1: mtvaf_layer_grads_t */);

/* ---- optimizer step ------------------------------------------------------------
 * AdamW exactly as torch.optim.AdamW, which the reference trainer builds (modules/train.py:887-926) and steps
 * (:621-625): decoupled weight decay, bias corrections passed in (bc1 = 1 - beta1^t, bc2_sqrt = sqrt(1 - beta2^t)).
 * mtvaf_adamw updates ONE flat fp32 tensor (an encoder layer's parameter buffer: all 16 parameters of a layer in one
 * launch, enqueued behind that layer's gradient all-reduce so the update overlaps the rest of the backward pass) and
 * optionally writes the updated parameters rounded to bf16 (the GEMM operand shadow of the bf16 compute mode);
 * max_blocks > 0 caps its grid (a background update that trickles under MFMA-bound kernels instead of taking the whole
 * HBM rate from them for its duration; 0 = full width).
 * mtvaf_adamw_multi updates `count` tensors of one parameter group per launch (host arrays of device pointers); every tensor is
 * checked before the first launch, so a refused call has written nothing.
 * The arithmetic of one element is the same in every mtvaf_adamw* entry point, on aligned and unaligned bases, each line ONE fp32
 * rounding (s = grad_scale, times the clip coefficient in the *_dev forms; omb = (float)(1 - beta); sqrt and / correctly rounded):
 *   gs = g * s;  d = fma(g, s, -m);  m = fma(omb1, d, m);  v = fma(beta2, v, gs * (omb2 * gs));
 *   p1 = fma(-(lr * wd), p, p);  den = sqrt(v) / bc2_sqrt + eps;  p = fma(-(lr / bc1), m / den, p1) */
int mtvaf_adamw(float* p, const float* g, float* m, float* v, long n, float lr, double beta1, double beta2, float eps,
                float weight_decay, float bc1, float bc2_sqrt, float grad_scale, void* p_bf16, int max_blocks,
                mtvaf_stream_t stream);
/* mtvaf_adamw over a flat buffer (n % 4 == 0, 16-byte aligned) that ALSO rewrites the plane images (the pre-split operand form of
 * csrc/gemm_f32p.hip, round 5) of nseg <= 4 row-major fp32 matrices inside it -- an encoder layer's wqkv / wo / w1 / w2: matrix s starts
 * at element seg_begin[s] (% 4 == 0), is [seg_rows[s]][seg_cols[s]] (cols % 32 == 0) and has its tile-blocked image
 * [cols / 32][3][rows][32] bf16 at seg_img[s].  The same update as mtvaf_adamw, bit for bit; the images match the updated weights. */
int mtvaf_adamw_planes(float* p, const float* g, float* m, float* v, long n, float lr, double beta1, double beta2, float eps,
                       float weight_decay, float bc1, float bc2_sqrt, float grad_scale, int nseg, const long* seg_begin,
                       const int* seg_rows, const int* seg_cols, void* const* seg_img, int max_blocks, mtvaf_stream_t stream);
int mtvaf_adamw_multi(int count, float* const* p, const float* const* g, float* const* m, float* const* v,
                      const long* n, float lr, double beta1, double beta2, float eps, float weight_decay, float bc1,
                      float bc2_sqrt, float grad_scale, mtvaf_stream_t stream);

/* ---- gradient clipping by global L2 norm, norm reporting and a non-finite skip, all on the device (new functionality: the
 * reference trainer does not clip, modules/train.py:620-625).  No host synchronisation, no atomics, no pass that rescales gradients.
 * mtvaf_grad_sqnorm_multi: sum of squares of `count` fp32 tensors (host arrays of device pointers and lengths, any count; pointers
 * 4-byte aligned).  Every tensor is cut into chunks of 65536 elements -- independent of the device and of the grid -- and one block
 * per chunk writes one double to its own slot of `partials`, tensor after tensor; squares and sums are double from the first
 * operation (a gradient of 1e20 gives a finite norm, and the result does not depend on the length of a run).
 * mtvaf_grad_sqnorm_workspace_bytes: the bytes of `partials` for these lengths (8 per chunk; 0 for a bad argument); fewer in the
 * call: MTVAF_ERR_WORKSPACE.
 * mtvaf_grad_clip_finalize (one block) adds `count` partials in index order and writes clip_state[4] (16-byte aligned):
 *   [0] norm = fp32(sqrt(sum))   [1] coef = min(1, max_norm / (norm + 1e-6)), torch's clip_grad_norm_ rule; 1 for max_norm <= 0
 *   [2] finite = 1.f / 0.f       [3] 0
 * A norm that is not finite in fp32, with skip_nonfinite != 0: coef = 0, finite = 0 and *skipped (int32, may be NULL) += 1.  With
 * skip_nonfinite == 0, finite stays 1 and the norm reaches coef as in torch (inf -> 0, NaN -> NaN).  Same inputs, same bits.
 * mtvaf_adamw_dev / _planes_dev / _multi_dev: the entry points above with the gradient scaled by grad_scale * clip_state[1]; with
 * clip_state[2] == 0 they write nothing (p, m, v, the bf16 shadow and the plane images keep their bits).  With coef == 1 they
 * equal their counterparts bit for bit. */
size_t mtvaf_grad_sqnorm_workspace_bytes(int count, const long* n);
int mtvaf_grad_sqnorm_multi(int count, const float* const* g, const long* n, void* partials, size_t partials_bytes,
                            mtvaf_stream_t stream);
int mtvaf_grad_clip_finalize(const void* partials, long count, float max_norm, int skip_nonfinite, float* clip_state,
                             int* skipped, mtvaf_stream_t stream);
int mtvaf_adamw_dev(float* p, const float* g, float* m, float* v, long n, float lr, double beta1, double beta2, float eps,
                    float weight_decay, float bc1, float bc2_sqrt, float grad_scale, void* p_bf16, int max_blocks,
                    const float* clip_state, mtvaf_stream_t stream);
int mtvaf_adamw_planes_dev(float* p, const float* g, float* m, float* v, long n, float lr, double beta1, double beta2, float eps,
                           float weight_decay, float bc1, float bc2_sqrt, float grad_scale, int nseg, const long* seg_begin,
                           const int* seg_rows, const int* seg_cols, void* const* seg_img, int max_blocks,
                           const float* clip_state, mtvaf_stream_t stream);
int mtvaf_adamw_multi_dev(int count, float* const* p, const float* const* g, float* const* m, float* const* v,
                          const long* n, float lr, double beta1, double beta2, float eps, float weight_decay, float bc1,
                          float bc2_sqrt, float grad_scale, const float* clip_state, mtvaf_stream_t stream);

/* ---- an exponential moving average (EMA) of the parameters, kept by the update kernels themselves (new functionality: the
 * reference trainer keeps none).  mtvaf_adamw_ema / _planes_ema / _multi_ema are the three updates above with one more fp32 buffer
 * per tensor, `ema` (as long as p, aligned like m and v), and ema_omd = 1 - decay in [0, 1]: after its update every element does
 *   ema = fmaf(ema_omd, p_new - ema, ema)
 * -- one more load and one more store (8 bytes per parameter) in the pass that already holds p_new in registers.  ema_omd == 1 makes
 * the average the new parameter exactly (how a zero-initialised average starts).  p, m, v, the bf16 shadow and the plane images are
 * the bits of the entry points without `ema`: the average feeds nothing.  clip_state NULL: the host-scalar form; otherwise the
 * *_dev form, and with clip_state[2] == 0 the average keeps its bits with everything else.  A NULL `ema` or an ema_omd outside
 * [0, 1]: MTVAF_ERR_ARG.
 * mtvaf_swap_f32_multi exchanges a[i] and b[i] (n[i] floats each, 4-byte aligned; host arrays of device pointers, any count) bit
 * for bit -- the parameters against their averages, and back.  A pair whose two sides overlap, a NULL pointer or n[i] <= 0:
 * MTVAF_ERR_ARG, and nothing is written. */
int mtvaf_adamw_ema(float* p, const float* g, float* m, float* v, long n, float lr, double beta1, double beta2, float eps,
                    float weight_decay, float bc1, float bc2_sqrt, float grad_scale, void* p_bf16, int max_blocks, float* ema,
                    float ema_omd, const float* clip_state, mtvaf_stream_t stream);
int mtvaf_adamw_planes_ema(float* p, const float* g, float* m, float* v, long n, float lr, double beta1, double beta2, float eps,
                           float weight_decay, float bc1, float bc2_sqrt, float grad_scale, int nseg, const long* seg_begin,
                           const int* seg_rows, const int* seg_cols, void* const* seg_img, int max_blocks, float* ema,
                           float ema_omd, const float* clip_state, mtvaf_stream_t stream);
int mtvaf_adamw_multi_ema(int count, float* const* p, const float* const* g, float* const* m, float* const* v,
                          const long* n, float lr, double beta1, double beta2, float eps, float weight_decay, float bc1,
                          float bc2_sqrt, float grad_scale, float* const* ema, float ema_omd, const float* clip_state,
                          mtvaf_stream_t stream);
int mtvaf_swap_f32_multi(int count, float* const* a, float* const* b, const long* n, mtvaf_stream_t stream);

/* ---- lr and weight decay that differ INSIDE one flat buffer (new functionality: the reference trains every parameter of the
 * encoder with one weight decay, modules/train.py:894-916; the usual BERT fine-tuning recipe exempts biases and LayerNorm weights).
 * mtvaf_adamw_seg / mtvaf_adamw_planes_seg are mtvaf_adamw / mtvaf_adamw_planes (same update, torch.optim.AdamW's, same reference
 * lines; bc1, bc2_sqrt, grad_scale, max_blocks as there) over a buffer cut into nseg consecutive segments: segment k is the elements
 * [seg_end[k-1], seg_end[k]) (from 0 for k == 0) and is updated with seg_lr[k] and seg_wd[k]; beta1, beta2, eps, the bias corrections
 * and grad_scale belong to the launch.  The three host arrays are read during the call (the table travels in the kernel arguments).
 * An element gets the bits mtvaf_adamw gives it when run on its segment alone with that segment's lr and weight decay.
 *   1 <= nseg <= 16; seg_end strictly increasing, seg_end[nseg - 1] == n, every other end a multiple of 4; otherwise MTVAF_ERR_ARG.
 *   n > 2^33 - 8: MTVAF_ERR_SHAPE.  p, g, m, v (and ema) 16-byte aligned, p_bf16 8-byte; n % 4 may be anything for mtvaf_adamw_seg.
 * The options of the unsegmented entry points are nullable arguments here, there is no _dev / _ema family:
 *   clip_state  NULL: host scalars only.  Otherwise the state of mtvaf_grad_clip_finalize: the gradient is scaled by grad_scale *
 *               clip_state[1], and with clip_state[2] == 0 the launch writes nothing.
 *   ema         NULL: no average (ema_omd is not read).  Otherwise ema = fmaf(ema_omd, p_new - ema, ema) as in mtvaf_adamw_ema;
 *               ema_omd outside [0, 1]: MTVAF_ERR_ARG.
 *   p_bf16      (mtvaf_adamw_seg) NULL or the bf16 shadow of the whole buffer.
 * mtvaf_adamw_planes_seg also rewrites the plane images of nmat <= 4 matrices inside the buffer, under the conditions of
 * mtvaf_adamw_planes (n % 4 == 0; mat_begin % 4 == 0, cols % 32 == 0, images 16-byte aligned: MTVAF_ERR_ALIGN / MTVAF_ERR_SHAPE as
 * there).  A matrix may lie across segment ends.  A refused call launches nothing. */
int mtvaf_adamw_seg(float* p, const float* g, float* m, float* v, long n, int nseg, const long* seg_end, const float* seg_lr,
                    const float* seg_wd, double beta1, double beta2, float eps, float bc1, float bc2_sqrt, float grad_scale,
                    void* p_bf16, int max_blocks, float* ema, float ema_omd, const float* clip_state, mtvaf_stream_t stream);
int mtvaf_adamw_planes_seg(float* p, const float* g, float* m, float* v, long n, int nseg, const long* seg_end, const float* seg_lr,
                           const float* seg_wd, double beta1, double beta2, float eps, float bc1, float bc2_sqrt, float grad_scale,
                           int nmat, const long* mat_begin, const int* mat_rows, const int* mat_cols, void* const* mat_img,
                           int max_blocks, float* ema, float ema_omd, const float* clip_state, mtvaf_stream_t stream);

/* ---- the step's own hyper-parameters on the device: an optimizer step that a graph capture can contain (new functionality: the
 * reference steps eagerly, modules/train.py:620-625).  Every entry point above takes lr, bc1, bc2_sqrt and ema_omd as host floats,
 * which a capture would freeze.  Here the host uploads ONE table for the whole run, a row of 24 bytes per optimizer step t = 1 .. rows:
 *   { double lr_factor;  float bc1, bc2_sqrt, ema_omd;  int32 pad; }
 * (lr_factor: what the lr schedule's lambda returns for the step whose lr update t uses; the floats exactly as the entry points above
 * would have been handed them at step t), and the update kernels read the row of the step being taken from a fixed 32-byte block:
 *   { double lr_factor;  float bc1, bc2_sqrt, ema_omd;  int32 overrun;  int64 step; }
 * mtvaf_adamw_sched_advance (one block, plain stores from one lane): *counter += 1 (device int64), row min(*counter, rows) - 1 ->
 * current, current.step = *counter, current.overrun = 1 when *counter lies outside 1 .. rows, else 0.  table, counter and current
 * 8-byte aligned (MTVAF_ERR_ALIGN), rows >= 1 (MTVAF_ERR_ARG).
 * mtvaf_adamw_sched / _planes_sched / _multi_sched / _seg_sched / _planes_seg_sched are mtvaf_adamw / _planes / _multi / _seg /
 * _planes_seg with
 *   lr = (float)(base_lr * current.lr_factor)   -- base_lr (per segment: seg_lr[k]) a DOUBLE: the product and the single rounding to
 *                                                  float of a LambdaLR followed by the float argument above, so the same bits
 *   bc1, bc2_sqrt, ema_omd                      -- read from current
 * and the same update otherwise, bit for bit.  current.overrun != 0: the launch writes nothing, exactly as clip_state[2] == 0.
 * Their options are nullable arguments as in mtvaf_adamw_seg: ema (mtvaf_adamw_multi_sched: a host array of device pointers) NULL: no
 * average; clip_state NULL: grad_scale alone; p_bf16 NULL: no shadow.  Shapes, alignments and error codes are those of the
 * counterparts; current NULL: MTVAF_ERR_ARG.  No argument changes from step to step. */
int mtvaf_adamw_sched_advance(const void* table, long rows, long* counter, void* current, mtvaf_stream_t stream);
int mtvaf_adamw_sched(float* p, const float* g, float* m, float* v, long n, double base_lr, double beta1, double beta2, float eps,
                      float weight_decay, float grad_scale, void* p_bf16, int max_blocks, float* ema, const float* clip_state,
                      const void* current, mtvaf_stream_t stream);
int mtvaf_adamw_planes_sched(float* p, const float* g, float* m, float* v, long n, double base_lr, double beta1, double beta2,
                             float eps, float weight_decay, float grad_scale, int nmat, const long* mat_begin, const int* mat_rows,
                             const int* mat_cols, void* const* mat_img, int max_blocks, float* ema, const float* clip_state,
                             const void* current, mtvaf_stream_t stream);
int mtvaf_adamw_multi_sched(int count, float* const* p, const float* const* g, float* const* m, float* const* v, const long* n,
                            double base_lr, double beta1, double beta2, float eps, float weight_decay, float grad_scale,
                            float* const* ema, const float* clip_state, const void* current, mtvaf_stream_t stream);
int mtvaf_adamw_seg_sched(float* p, const float* g, float* m, float* v, long n, int nseg, const long* seg_end, const double* seg_lr,
                          const float* seg_wd, double beta1, double beta2, float eps, float grad_scale, void* p_bf16, int max_blocks,
                          float* ema, const float* clip_state, const void* current, mtvaf_stream_t stream);
int mtvaf_adamw_planes_seg_sched(float* p, const float* g, float* m, float* v, long n, int nseg, const long* seg_end,
                                 const double* seg_lr, const float* seg_wd, double beta1, double beta2, float eps, float grad_scale,
                                 int nmat, const long* mat_begin, const int* mat_rows, const int* mat_cols, void* const* mat_img,
                                 int max_blocks, float* ema, const float* clip_state, const void* current, mtvaf_stream_t stream);

/* ---- bf16 gradient wire format of the data-parallel exchange (mtvaf_amd/parallel.py; new functionality, the
 * reference never synchronises gradients: MTVAF_training.py:305-309).  pack: dst[i] = bf16(src[i]), zero padding up to
 * npad (npad % 8 == 0); reduce: out[c] = bf16(scale * sum_r recv[r*chunk + c]) with fp32 accumulation in rank order;
 * unpack: dst[i] = float(src[i]).  The collectives themselves (all_to_all, all_gather: RCCL over xGMI) are issued
 * through torch.distributed -- the section 8(b) proposal of mtvaf_rccl_* entry points is not built, see INTEGRATION.md. */
int mtvaf_grad_pack_bf16(const float* src, void* dst, long n, long npad, mtvaf_stream_t stream);
int mtvaf_grad_reduce_bf16(const void* recv, void* out, int world, long chunk, float scale, mtvaf_stream_t stream);
int mtvaf_grad_unpack_bf16(const void* src, float* dst, long n, mtvaf_stream_t stream);

/* ---- Adversarial perturbation of the embedding output: one FGM / PGD / FreeLB step (mtvaf_amd/adversarial.py; new
 * functionality, the reference trainer has no adversarial step).  g [B,S,H] fp32: the gradient at the embedding output;
 * mask [B,S] u8, non-zero = live, any pattern; delta_in [B,S,H] or NULL; x [B,S,H] or NULL.  A unit u is all live rows
 * of a sentence (scope SENTENCE) or one live row (scope TOKEN), |.|_u its L2 norm:
 *   norm L2,   delta_in NULL:  delta_out = eps * g / |g|_u
 *   norm L2,   delta_in:       d = delta_in + step * g / |g|_u;  if |d|_u > eps: d *= eps / |d|_u;  delta_out = d
 *   norm LINF, delta_in NULL:  delta_out = eps * sign(g)          (sign(0) = 0)
 *   norm LINF, delta_in:       delta_out = clamp(delta_in + step * sign(g), -eps, eps)
 * Rows with mask 0 are exact 0.0f in delta_out whatever g and delta_in hold there (neither is read).  A unit whose |g|_u
 * is 0, inf or NaN -- as rounded to fp32 -- takes no gradient term: delta_out = 0 without delta_in, the projected (L2) or
 * clamped (LINF) delta_in with it; a finite delta_in gives a finite delta_out.  out [B,S,H] (optional, needs x) =
 * x + delta_out, bit for bit the fp32 sum of the stored delta.  stats [B,2] = {|g| over the sentence's live rows,
 * |delta_out| over the sentence}, for either scope; a non-finite |g| is reported there.  delta_out may be delta_in.
 * Squares and sums run in double from the first operation and are rounded to fp32 once; per element the fp32 work is one
 * division and one multiplication, so g * 2^k (nothing underflowing) gives the same bits.  No atomics, no host
 * synchronisation: the same inputs give the same bits.  workspace: mtvaf_adv_workspace_bytes(B, S) bytes, 8-byte
 * aligned (MTVAF_ERR_WORKSPACE if short).  B >= 1, 1 <= S <= 512, 1 <= H <= 1024 (MTVAF_ERR_SHAPE); eps, step finite
 * and >= 0, norm / scope one of the constants (MTVAF_ERR_ARG): checked before any launch.
 * mtvaf_adv_add: out[i] = x[i] + delta[i], n elements (the embedding tap's forward, engine.EmbeddingTapFunction). */
#define MTVAF_ADV_NORM_L2 0
#define MTVAF_ADV_NORM_LINF 1
#define MTVAF_ADV_SCOPE_SENTENCE 0
#define MTVAF_ADV_SCOPE_TOKEN 1
size_t mtvaf_adv_workspace_bytes(int B, int S);
int mtvaf_adv_perturb(const float* g, const float* delta_in, const float* x, const uint8_t* mask, float* delta_out,
                      float* out, float* stats, int B, int S, int H, float eps, float step, int norm, int scope,
                      void* workspace, size_t workspace_bytes, mtvaf_stream_t stream);
int mtvaf_adv_add(const float* x, const float* delta, float* out, long n, mtvaf_stream_t stream);

/* ---- Sharpness-aware minimisation (SAM, Foret et al. 2021): the ascent step in weight space and the way back
 * (mtvaf_amd/optim.py AdamW(sam_rho=...), mtvaf_amd/sam.py; new functionality, the reference trainer has nothing like it).
 * Streaming kernels, no atomics, no host synchronisation: the same inputs give the same bits.
 * mtvaf_sam_finalize (one block) adds the `count` double partials of mtvaf_grad_sqnorm_multi in index order and writes
 * sam_state[4] (16-byte aligned):
 *   [0] norm = fp32(sqrt(sum))   [1] scale = (float)(rho / (sqrt(sum) + 1e-12)), quotient and sum in double
 *   [2] finite = 1.f / 0.f       [3] 0
 * A norm that is not finite in fp32: scale = 0, finite = 0 and *skipped (int32, may be NULL) += 1.  rho finite and >= 0.
 * mtvaf_sam_perturb: for every element  backup = p;  p = fmaf(sam_state[1], g, p)  -- one correctly rounded operation.  Any n,
 * pointers 4-byte aligned; p_bf16 NULL or the bf16 shadow of the buffer, which receives the new p rounded as mtvaf_adamw rounds it.
 * With sam_state[2] == 0 p keeps its bits (g is not read), and backup and the shadow are still written, from that unchanged p.
 * mtvaf_sam_perturb_planes: the same over a flat buffer (n % 4 == 0; p, g, backup 16-byte aligned) that also rewrites the plane
 * images of the nseg <= 4 matrices inside it; seg_begin / seg_rows / seg_cols / seg_img and the image layout are those of
 * mtvaf_adamw_planes.  With sam_state[2] == 0 the images are written from the unchanged p.
 * mtvaf_sam_perturb_multi: `count` tensors per call (host arrays of device pointers and lengths, any count: 48 per launch).
 * mtvaf_sam_restore / _restore_planes / _restore_multi: p = backup bit for bit; the first two rewrite the shadow / the plane
 * images from the restored values.  All three perturb forms give a buffer the same bits.
 * Errors, checked before anything is launched: a NULL pointer (p_bf16 and skipped excepted), n <= 0, a misaligned pointer or
 * length, p / backup (or g) ranges that overlap: MTVAF_ERR_ARG; a matrix table mtvaf_adamw_planes would refuse:
 * MTVAF_ERR_ARG / MTVAF_ERR_SHAPE as there. */
int mtvaf_sam_finalize(const void* partials, long count, float rho, float* sam_state, int* skipped, mtvaf_stream_t stream);
int mtvaf_sam_perturb(float* p, const float* g, float* backup, long n, const float* sam_state, void* p_bf16,
                      mtvaf_stream_t stream);
int mtvaf_sam_perturb_planes(float* p, const float* g, float* backup, long n, const float* sam_state, int nseg,
                             const long* seg_begin, const int* seg_rows, const int* seg_cols, void* const* seg_img,
                             mtvaf_stream_t stream);
int mtvaf_sam_perturb_multi(int count, float* const* p, const float* const* g, float* const* backup, const long* n,
                            const float* sam_state, mtvaf_stream_t stream);
int mtvaf_sam_restore(float* p, const float* backup, long n, void* p_bf16, mtvaf_stream_t stream);
int mtvaf_sam_restore_planes(float* p, const float* backup, long n, int nseg, const long* seg_begin, const int* seg_rows,
                             const int* seg_cols, void* const* seg_img, mtvaf_stream_t stream);
int mtvaf_sam_restore_multi(int count, float* const* p, const float* const* backup, const long* n, mtvaf_stream_t stream);

/* ---- Word-level tagging head: the word axis of a batch, piece-to-word pooling and its backward (mtvaf_amd/words.py,
 * engine.WordPoolFunction; new functionality, the reference tags word pieces).  No atomics, no host synchronisation, every
 * element of every output written: the same inputs give the same bits.
 * mtvaf_word_index: attention_mask [B,S] u8, a prefix mask (len = its leading non-zero entries); token_to_word [B,S] int32, -1
 * outside the map (mtvaf_amd.spans.batch_token_to_word).  Token s < len OPENS a column iff s == 0, map[s] < 0 or
 * map[s] != map[s-1]; map entries at s >= len are never read.  For the caller's width W >= 1 (S always suffices):
 *   col_start [B,W] int32  first token of the column (0 for a dead column)     col_len [B,W] int32  its tokens, 0 = no column
 *   col_of_token [B,S] int32  the token's column; -1 for s >= len and for tokens of columns >= W
 *   word_mask [B,W] u8  1 on live columns (a prefix mask)     word_id [B,W] int32  the column's map value, -1 if unmapped / dead
 *   n_cols [B] int32  the true column count: it may exceed W, the columns beyond W are dropped
 * B >= 1, 1 <= S <= 512, W >= 1 (MTVAF_ERR_SHAPE); int32 pointers 4-byte aligned (MTVAF_ERR_ALIGN).
 * mtvaf_word_pool_fwd: x [B,S,H] fp32 -> y [B,W,H] fp32.  FIRST / LAST: the column's first / last piece, copied.  MEAN: the
 * pieces added one after the other in ascending token order in fp32, then one correctly rounded division by (float)col_len (no
 * reciprocal, no contraction).  Dead columns (col_len 0, or a start / length outside the sentence) are exact zeros; x is read
 * only inside live columns.
 * mtvaf_word_pool_bwd: dy [B,W,H] -> dx [B,S,H], a gather: the selected piece gets its column's dy (FIRST / LAST), every piece
 * dy / (float)col_len (MEAN, the same division); tokens with col_of_token < 0 and unselected pieces get exact zeros; dy is
 * read only at live columns.
 * Both: 16-byte accesses when H % 4 == 0 and x, y (dy, dx) are 16-byte aligned, scalar accesses otherwise, the same values.
 * B, S, W, H >= 1 (MTVAF_ERR_SHAPE); a NULL pointer or an unknown mode: MTVAF_ERR_ARG; 4-byte alignment: MTVAF_ERR_ALIGN. */
#define MTVAF_WORD_POOL_FIRST 0
#define MTVAF_WORD_POOL_LAST 1
#define MTVAF_WORD_POOL_MEAN 2
int mtvaf_word_index(const uint8_t* attention_mask, const int* token_to_word, int* col_start, int* col_len, int* col_of_token,
                     uint8_t* word_mask, int* word_id, int* n_cols, int B, int S, int W, mtvaf_stream_t stream);
int mtvaf_word_pool_fwd(const float* x, const int* col_start, const int* col_len, float* y, int B, int S, int W, int H, int mode,
                        mtvaf_stream_t stream);
int mtvaf_word_pool_bwd(const float* dy, const int* col_start, const int* col_len, const int* col_of_token, float* dx, int B,
                        int S, int W, int H, int mode, mtvaf_stream_t stream);

/* ---- Layer mix: a learned weighted sum of hidden states for the heads (mtvaf_amd/modules/layer_mix.py,
 * engine.EncoderMixFunction; new functionality, the reference's heads read the last layer).  states: a HOST array of K device
 * pointers, each [rows,H] fp32 (the residual-stream states of the chosen layers, in ascending layer order); scalars [K] and
 * gamma [1] fp32 ON THE DEVICE.  No atomics, no host synchronisation, a launch geometry that depends on (rows, H, K) alone: the
 * same inputs give the same bits.
 * mtvaf_layer_mix_fwd: y[r,c] = gamma * sum_j s_j h_j[r,c] with s = softmax(scalars): e_j = expf(scalars_j - max), their sum
 * taken in the order j = 0 .. K-1, s_j = e_j / sum (one correctly rounded division); the weighted sum is
 * fmaf(s_j, h_j, acc) from acc = 0 in the order j = 0 .. K-1, multiplied by gamma once at the end.  Rows are independent.
 * mtvaf_layer_mix_dots: with t_j = sum_{r,c} dy h_j, accumulated in double in two deterministic stages (one partial per block
 * and state in `workspace`, then a fixed-order sum), writes
 *   dgamma [1] = sum_j s_j t_j     dscalars [K]: gamma s_j (t_j - sum_i s_i t_i)     coef [K]: c_j = gamma * s_j (fp32),
 * the coefficient of dy in the gradient of state j.  workspace: at least MTVAF_LAYER_MIX_WORKSPACE_BYTES, 8-byte aligned.
 * mtvaf_layer_mix_inject: dh = fmaf(coef[j], dy, dh) (accumulate != 0) or dh = coef[j] * dy (accumulate == 0, dh is not read),
 * [rows,H] each; coef is read on the device.
 * Errors, checked before anything is launched: K outside 1 .. MTVAF_LAYER_MIX_MAX_K, j outside 0 .. K-1, a NULL pointer (an entry
 * of `states` included) or H % 4 != 0: MTVAF_ERR_ARG; rows < 1 or H < 4: MTVAF_ERR_SHAPE; a short workspace:
 * MTVAF_ERR_WORKSPACE; states, y, dy, dh not 16-byte aligned (the small vectors: 4-byte): MTVAF_ERR_ALIGN. */
#define MTVAF_LAYER_MIX_MAX_K 32
#define MTVAF_LAYER_MIX_DOT_BLOCKS 1024
#define MTVAF_LAYER_MIX_WORKSPACE_BYTES 262144 /* MAX_K x DOT_BLOCKS doubles */
int mtvaf_layer_mix_fwd(const float* const* states, int K, const float* scalars, const float* gamma, float* y, long rows, int H,
                        mtvaf_stream_t stream);
int mtvaf_layer_mix_dots(const float* const* states, int K, const float* dy, const float* scalars, const float* gamma, long rows,
                         int H, void* workspace, long workspace_bytes, float* dscalars, float* dgamma, float* coef,
                         mtvaf_stream_t stream);
int mtvaf_layer_mix_inject(const float* coef, int j, int K, const float* dy, float* dh, long rows, int H, int accumulate,
                           mtvaf_stream_t stream);

/* ---- masked-LM head (csrc/mlm.hip) ---------------------------------------------------------------------
 * replaces the host collator's masking (HF DataCollatorForLanguageModeling.torch_mask_tokens) and BertLMPredictionHead's decoder +
 * CrossEntropyLoss (modeling_bert.py, BertForMaskedLM) at vocabulary width.  All results are pure functions of their inputs: no
 * atomics, fixed reduction orders, nothing read back to the host; `count` is always a device word.
 *
 * mtvaf_uniform_fill: out[i] = 24 random bits * 2^-24 in [0, 1), a function of (seed, offset, i) on the dropout generator
 * (Philox4x32-10, and the registered device epoch if any).
 * mtvaf_mlm_mask: input_ids [B,S] int64; live [B,S] u8 (non-zero = attended; any pattern); special_mask [B,S] u8 or NULL (non-zero =
 * never selected); special_ids: n_special <= 8 ids on the HOST that are never selected; uniforms [B,S,3].  A live non-special token is
 * selected iff u0 < probability; a selected token becomes mask_token_id if u1 < 0.8, else min(V - 1, (int)(u2 * V)) if u1 < 0.9, else
 * stays.  Selected tokens are numbered in row-major order; the first `capacity` of them give positions [capacity] int32 (flat
 * b * S + t, ascending; -1 from *count on), labels [capacity] int64 (the original id; -100 from *count on) and are corrupted in
 * ids_out [B,S]; later ones stay unmasked and unpredicted.  count [1] int32 = min(selected, capacity); stats [3] int32 = eligible
 * tokens, selected tokens, selected tokens dropped for capacity.  workspace: mtvaf_mlm_mask_workspace_bytes(B) bytes.
 * mtvaf_scatter_rows: the backward of mtvaf_gather_rows for DISTINCT rows: dsrc [rows_src,H] = 0, then dsrc[map[r]] = d[r] for
 * every map[r] in [0, rows_src). */
int mtvaf_uniform_fill(float* out, long n, uint64_t seed, uint64_t offset, mtvaf_stream_t stream);
size_t mtvaf_mlm_mask_workspace_bytes(int B);
int mtvaf_mlm_mask(const int64_t* input_ids, const uint8_t* live, const uint8_t* special_mask, const float* uniforms,
                   const int64_t* special_ids, int n_special, float probability, long mask_token_id, int vocab_size, int capacity,
                   int64_t* ids_out, int* positions, int64_t* labels, int* count, int* stats, void* workspace, size_t workspace_bytes,
                   int B, int S, mtvaf_stream_t stream);
int mtvaf_scatter_rows(const float* d, const int* map, float* dsrc, int rows, int rows_src, int H, mtvaf_stream_t stream);
/* out = dy * gelu_erf'(pre), n % 4 == 0 elements, 16-byte aligned: what MTVAF_EPI_DGELU applies, for a gradient that comes out of
 * a row kernel (the LayerNorm backward of BertPredictionHeadTransform) and not out of a product. */
int mtvaf_dgelu(const float* dy, const float* pre, float* out, long n, mtvaf_stream_t stream);
/* Cross entropy over V classes from logits that exist one chunk [R, v1 - v0] at a time (row stride ld floats; the caller's GEMM
 * wrote x . W[v0:v1]^T into it, bias [V] or NULL is added here).  A row is live iff row < *count and 0 <= labels[row] < V; dead
 * rows are never read.  state: 4 R words (running maximum m, s = sum exp(l - m), the label's logit, the first index attaining m as
 * int32), started by the chunk with v0 == 0 and folded in ASCENDING chunk order, one rescale of s per chunk; only l - m <= 0 is
 * exponentiated.  mtvaf_vocab_ce_finish: loss_row [R] = m + log s - l_label and lse_row [R] (0 on dead rows); loss [1] = their sum
 * in double and fixed order, divided by the live rows for reduction 0 (mean; +0.0 without live rows), as it is for reduction 1
 * (sum); stats [3] int32 = live rows, rows whose first maximum is the label, rows below *count whose label is outside [0, V) and
 * not -100.  mtvaf_vocab_ce_chunk_bwd, in place on a recomputed chunk: dl = g_row (exp(l + bias - lse_row) - [v == label]), exact
 * zeros on dead rows; g_row = grad_rows[row], or *grad_out (divided by stats[0] for reduction 0) -- exactly one of the two is given.
 * mtvaf_vocab_ce_workspace_bytes: one logits chunk [R, chunk] and the state -- no term in V. */
size_t mtvaf_vocab_ce_workspace_bytes(int R, int H, int V, int chunk);
int mtvaf_vocab_ce_chunk_fwd(const float* logits, int ld, const float* bias, const int64_t* labels, const int* count, float* state,
                             int R, int V, int v0, int v1, mtvaf_stream_t stream);
int mtvaf_vocab_ce_finish(const float* state, const int64_t* labels, const int* count, float* loss, float* loss_row, float* lse_row,
                          int* stats, int R, int V, int reduction, mtvaf_stream_t stream);
int mtvaf_vocab_ce_chunk_bwd(float* logits, int ld, const float* bias, const int64_t* labels, const int* count, const float* lse_row,
                             const float* grad_out, const float* grad_rows, const int* stats, int R, int V, int v0, int v1,
                             int reduction, mtvaf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MTVAF_HIP_H */
