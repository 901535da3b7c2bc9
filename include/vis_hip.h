/* vis_hip.h - C ABI of libvis_hip.so, the MI355X (gfx950) compute library behind
 * the Inspector/Auditor "image -> defect report" step.
 *
 * The reference (Aditya-Somasi/Vision-Inspection-System) has no FFI of its own:
 * its hot path is one remote call,
 *     client.chat.completions.create(model=, messages=, temperature=, max_tokens=)
 *     (src/agents/vlm_inspector.py:105-111, src/agents/vlm_auditor.py:117-129,:152-158)
 * and everything the remote service does for that call (image patch embedding,
 * ViT, merger, LLM prefill, greedy decode) is what these entry points compute
 * locally.  The arithmetic each entry point replaces is cited against the
 * model definition the service runs (TF = transformers/models/qwen2_vl).
 *
 * Conventions
 *  - plain pointers and sizes only; every pointer is a DEVICE pointer unless
 *    stated otherwise; bf16 tensors are raw uint16 bit patterns;
 *  - no allocation, no global state, no synchronisation: kernels are enqueued
 *    on `stream` (a hipStream_t passed as void*) and may be captured in a hipGraph;
 *  - return value: 0 = enqueued, 1 = argument/shape/alignment precondition
 *    violated (nothing launched), 2 = HIP launch error, 3 = valid arguments but
 *    this kernel form does not cover the shape on this device (nothing launched;
 *    the caller issues the equivalent separate launches - vis_decode_chain only).
 */
#ifndef VIS_HIP_H
#define VIS_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef void* vis_stream_t; /* hipStream_t */

#define VIS_OK 0
#define VIS_ERR_ARG 1
#define VIS_ERR_LAUNCH 2
#define VIS_ERR_UNSUPPORTED 3

/* activation selectors for vis_gemm_bf16 / vis_gemv_bf16 */
#define VIS_ACT_NONE 0
#define VIS_ACT_QUICKGELU 1 /* x * sigmoid(1.702 x)      ViT MLP (hidden_act="quick_gelu")   */
#define VIS_ACT_GELU_ERF 2  /* 0.5 x (1 + erf(x/sqrt2))  merger nn.GELU(), TF modeling:284   */
#define VIS_ACT_SWIGLU 3    /* silu(gate) * up over a 16-row interleaved gate/up weight       */

int vis_abi_version(void);

/* K2  C[M,N] = act(A[M,K] * W[N,K]^T + bias[N]) + R[M,N]      (bf16 in/out, f32 accumulate)
 * Replaces nn.Linear / Conv3d-as-GEMM in TF modeling_qwen2_vl.py:251-274 (patch embed),
 * :281-286 (merger), :296-298 (ViT MLP), :349-350,:421 (ViT qkv/proj), :459-466 (LLM MLP),
 * :501-504,:555 (LLM q/k/v/o).  K % 64 == 0, N % 4 == 0, lda/ldw % 8 == 0.
 * VIS_ACT_SWIGLU: W rows are [gate 16 | up 16] interleaved, output has N/2 columns. */
int vis_gemm_bf16(const void* A, const void* W, const void* bias, const void* R, void* C,
                  int M, int N, int K, int lda, int ldw, int ldc, int ldr, int act, vis_stream_t stream);

/* K3  y = w * bf16(x * rsqrt(mean(x^2) + eps))          TF modeling_qwen2_vl.py:96-110  */
int vis_rmsnorm_bf16(const void* x, const void* w, void* y, int rows, int N, int ldx, int ldy,
                     float eps, vis_stream_t stream);

/* K3 over the heads of a packed row: x [tokens][ldx] holds `heads` consecutive head_dim (= 128) wide heads per token; every
 * (token, head) slice is normalised with the one weight w [128] (mllama k_norm on the cross-attention keys, TF:models/mllama/
 * modeling_mllama.py:411-440).  Per slice bit-identical to vis_rmsnorm_bf16 on x[:, 128 h ..]; one launch instead of `heads`. */
int vis_rmsnorm_heads_bf16(const void* x, const void* w, void* y, int tokens, int heads, int head_dim, int ldx, int ldy,
                           float eps, vis_stream_t stream);

/* K5  y = (x - mean) * rsqrt(var + eps) * w + b         TF modeling_qwen2_vl.py:281,:428-429 */
int vis_layernorm_bf16(const void* x, const void* w, const void* b, void* y, int rows, int N,
                       int ldx, int ldy, float eps, vis_stream_t stream);

/* K4  rotary embedding + head split (+ KV-cache write, + V transpose).
 * qkv[S, (Hq+2Hkv)*HD] packed projections; cos/sin [S, HD] f32 rows (M-RoPE sections already
 * selected per channel, TF modeling_qwen2_vl.py:180-222; ViT 2-D rope :225-236).
 * q -> [Hq][S][HD]; k,v -> [Hkv][k_tokens][HD] rows k_pos0.. (v may be NULL);
 * vt -> [Hkv][HD][vt_ld] keys contiguous (may be NULL), in the k-slot column order vis_attn_prefill reads: inside
 * every aligned group of 32 keys, key 16a + 4h + r (a < 2, h < 4, r < 4) is column 8h + 4a + r (ABI version 2).
 * HD in {128, 80}.
 * Hq == 0 (k/v only) or Hkv == 0 (q only) give a partial split; cosv == sinv == NULL means no rotation (mllama
 * vision tower and cross-attention operands, TF:models/mllama/modeling_mllama.py:234-268,:411-440). */
int vis_qkv_rope_split(const void* qkv, const void* cosv, const void* sinv, void* q, void* k, void* v,
                       void* vt, int S, int ld_qkv, int Hq, int Hkv, int HD, int k_tokens, int k_pos0,
                       int vt_ld, vis_stream_t stream);

/* vis_qkv_rope_split for the nreq (<= 8) requests of one prompt-pass group as ONE launch (the engine's stacked suffix pass,
 * replacing the per-image loop of /root/reference/src/orchestration/graph.py:308-357 one level down): request r reads the S rows at
 * qkv + r * qkv_bs (same cos / sin rows for all: the requests share their prompt structure) and writes q + r * q_bs,
 * k + kv_off[r] and v + kv_off[r] (element offsets of its cache slot; HOST array of nreq values), vt + r * vt_bs.  Strides and
 * offsets in elements, multiples of 8.  Per request bit-identical to vis_qkv_rope_split. */
int vis_qkv_rope_split_many(const void* qkv, const void* cosv, const void* sinv, void* q, void* k, void* v, void* vt, int S,
                            int ld_qkv, int Hq, int Hkv, int HD, int k_tokens, int k_pos0, int vt_ld, int nreq,
                            long long qkv_bs, long long q_bs, long long vt_bs, const long long* kv_off, vis_stream_t stream);

/* K6/K7  flash-style prefill attention over a host-built work list of
 * {q0, qn<=128, k0, k1} int4 tiles (device memory): ViT varlen segments (cu_seqlens,
 * TF modeling_qwen2_vl.py:356-423) and LLM causal GQA prefill (:508-556).
 * O[Sq][ldo], column head*HD + d.  softmax(QK^T * scale) V, f32 softmax. */
int vis_attn_prefill(const void* Q, const void* K, const void* Vt, void* O, const void* work, int n_work,
                     int Hq, int Hkv, int HD, int Sq, int k_tokens, int vt_ld, int ldo, int causal,
                     float scale, vis_stream_t stream);
/* Same with a row offset: the work items' query rows (and the causal rule key <= query) are positions of the whole
 * sequence, Q / O hold only rows q_row0 .. q_row0 + Sq - 1 - the prompt pass of a request whose first q_row0 tokens
 * (the text prefix the reference puts in front of the image, src/agents/vlm_inspector.py:462-470, identical for the
 * images of a batch) were computed once and copied into its KV cache. */
int vis_attn_prefill_rows(const void* Q, const void* K, const void* Vt, void* O, const void* work, int n_work,
                          int Hq, int Hkv, int HD, int Sq, int k_tokens, int vt_ld, int ldo, int causal,
                          float scale, int q_row0, vis_stream_t stream);

/* vis_attn_prefill_rows (HD = 128) for the nreq (<= 8) requests of one prompt-pass group as ONE launch: request r reads Q + r * q_bs,
 * K + kv_off[r] (HOST array, element offsets), Vt + r * vt_bs and work items [r * n_work, (r + 1) * n_work) - one list per request
 * (the mllama cross-attention's key counts differ per image) - and writes O + r * o_bs.  Per request bit-identical. */
int vis_attn_prefill_rows_many(const void* Q, const void* K, const void* Vt, void* O, const void* work, int n_work, int Hq,
                               int Hkv, int HD, int Sq, int k_tokens, int vt_ld, int ldo, int causal, float scale, int q_row0,
                               int nreq, long long q_bs, long long vt_bs, long long o_bs, const long long* kv_off,
                               vis_stream_t stream);

/* K7, balanced form (HD = 128, causal, keys from 0): work = n_work x int4 {qB0, qBn, qA0, qAn}, a late and an early
 * 128-row query block of one sequence per 512-thread workgroup (qAn = 0: none), so that every workgroup of the causal
 * grid carries the same number of key tiles.  Results equal vis_attn_prefill_rows(..., causal = 1). */
int vis_attn_prefill_pairs(const void* Q, const void* K, const void* Vt, void* O, const void* work, int n_work,
                           int Hq, int Hkv, int HD, int Sq, int k_tokens, int vt_ld, int ldo, float scale,
                           int q_row0, vis_stream_t stream);

/* vis_attn_prefill_pairs for the nreq (<= 8) requests of one prompt-pass group as ONE launch (same work list): request r reads
 * Q + r * q_bs, K + kv_off[r] (HOST array, element offsets), Vt + r * vt_bs and writes O + r * o_bs.  Per request bit-identical to
 * vis_attn_prefill_pairs; the grid grows from Hq x n_work (168 workgroups for a 1289-row suffix) to Hq x n_work x nreq. */
int vis_attn_prefill_pairs_many(const void* Q, const void* K, const void* Vt, void* O, const void* work, int n_work, int Hq,
                                int Hkv, int HD, int Sq, int k_tokens, int vt_ld, int ldo, float scale, int q_row0, int nreq,
                                long long q_bs, long long vt_bs, long long o_bs, const long long* kv_off, vis_stream_t stream);

/* K6, key-split form (HD = 80, non-causal: the ViT towers).  Work items as in vis_attn_prefill plus SPLIT items, whose
 * y field is qn | (1 | part << 1 | pair << 2) << 8: parts 0 and 1 of pair `pair` cover the same query rows and the two
 * halves of their key range (cut at a multiple of 64); the kernel merges them (the later workgroup adds the earlier
 * one's partial, fixed operand order).  One 1024 x 1024 image at 16 heads leaves some SIMDs three 32-row blocks and
 * others two; with 9 of its 39 row blocks split every CU holds two whole and one half workgroup.
 * ws: vis_attn_split_ws_bytes(n_pairs, Hq) bytes, 256-byte aligned, zero before its first use (the kernel leaves it
 * reusable); one launch at a time per workspace.  Same reference as vis_attn_prefill (TF modeling_qwen2_vl.py:349-421). */
int vis_attn_split_ws_bytes(int n_pairs, int Hq);
int vis_attn_prefill_split(const void* Q, const void* K, const void* Vt, void* O, const void* work, int n_work,
                           int Hq, int Hkv, int HD, int Sq, int k_tokens, int vt_ld, int ldo, float scale,
                           int n_pairs, void* ws, long long ws_bytes, vis_stream_t stream);

/* K10  y[N] = act(W[N,K] x[K] + bias) + R, optional fused RMSNorm of x (norm_w != NULL).
 * out_f32 != 0 writes float logits (lm_head).  One generated token streams every weight once. */
int vis_gemv_bf16(const void* x, const void* W, const void* bias, const void* R, const void* norm_w,
                  void* y, int N, int K, int ldw, int act, int out_f32, float eps, vis_stream_t stream);

/* K4 + K11 (decode)  one launch per layer for the single new token: M-RoPE of q,k from the packed
 * projection row (cos/sin row *step_ptr of the [cache_tokens][128] f32 tables), KV-cache append at slot
 * *step_ptr, GQA attention over the *step_ptr + 1 cached keys split nsplit ways over the context
 * (nsplit * 128 >= cache_tokens), then a combine launch.  step_ptr is a device int: graph-replayable.
 * Workspaces: part_o [Hq][nsplit][128] f32, part_ml [Hq][nsplit][2] f32.  out: [Hq*128] bf16.
 * Replaces TF modeling_qwen2_vl.py:180-222 + :508-556 for q_len == 1 with a KV cache. */
int vis_decode_attn(const void* qkv, const void* cos_t, const void* sin_t, void* k_cache, void* v_cache,
                    const void* step_ptr, void* part_o, void* part_ml, void* out, int Hq, int Hkv, int HD,
                    int cache_tokens, int nsplit, float scale, int batch, long long qkv_bs, long long cache_bs,
                    long long tab_bs, vis_stream_t stream);
/* batch > 1: sequence b uses qkv + b*qkv_bs, caches + b*cache_bs, tables + b*tab_bs (element strides),
 * step_ptr[b], part_o/part_ml/out blocks of Hq*nsplit*128 / Hq*nsplit*2 / Hq*128 elements. */

/* vis_decode_attn for a batch whose sequences share their first shared_len cached keys (a multiple of 64: the common text
 * prefix of a batch inspection - the reference sends the text part first, src/agents/vlm_inspector.py:462-470 - which the
 * prompt passes copied into every slot): every sequence reads those keys / values from sequence 0's cache (one HBM read +
 * L2 hits instead of `batch` HBM reads of identical rows).  Bit-identical to vis_decode_attn. */
int vis_decode_attn_shared(const void* qkv, const void* cos_t, const void* sin_t, void* k_cache, void* v_cache,
                           const void* step_ptr, void* part_o, void* part_ml, void* out, int Hq, int Hkv, int HD,
                           int cache_tokens, int nsplit, float scale, int batch, long long qkv_bs, long long cache_bs,
                           long long tab_bs, int shared_len, vis_stream_t stream);

/* vis_decode_attn_shared with the qkv row finalised inside the attention launch: `part` = the ksplit f32 partial slabs
 * [slab_rows][(Hq + 2 Hkv) * 128] the batched qkv projection (vis_gemm_decode_bf16 / _fp8) left (slab_rows = 16 / 32 / 64 for batch
 * <= 16 / <= 32 / beyond), `bias` [n] or NULL, `sx` [batch] / `sw` [n] the e4m3 scales of fp8 partials or both NULL.  Column n of
 * sequence b = bf16(sum_k part[k][b][n] (* sx[b] * sw[n]) + bias[n]): vis_skinny_finalize's arithmetic bit for bit, i.e. the pair
 * (vis_skinny_finalize[_fp8], vis_decode_attn_shared) as ONE launch.  shared_len as above (0: none). */
int vis_decode_attn_parts(const void* part, int ksplit, int slab_rows, const void* bias, const void* sx, const void* sw,
                          const void* cos_t, const void* sin_t, void* k_cache, void* v_cache, const void* step_ptr,
                          void* part_o, void* part_ml, void* out, int Hq, int Hkv, int HD, int cache_tokens, int nsplit,
                          float scale, int batch, long long cache_bs, long long tab_bs, int shared_len, vis_stream_t stream);

/* vis_decode_attn_shared / vis_decode_attn_parts with the shared range named per sequence, in DEVICE memory (int32 [batch]
 * each, so one captured graph serves every layout): sequence b reads keys / values [0, fork_len[b]) from sequence parent[b]'s
 * cache and everything from fork_len[b] on - the streaming form's early prefetch, the KV append and the new token included -
 * from its own.  The n choices of one request are forks of the slot that ran its prompt pass; a batch's common text prefix is
 * "parent 0, fork_len P".  Contract (the caller's): fork_len[b] % 64 == 0, parent[parent[b]] == parent[b], the parent holds
 * rows [0, fork_len[b]) itself, the new token's slot >= fork_len[b].  The kernels clamp parent into [0, batch) and round
 * fork_len down to a multiple of 64 inside [0, cache_tokens): no table content forms an address outside the caches.
 * Same arithmetic, key order and split plan as the unforked entry points: bit-identical to vis_decode_attn /
 * vis_decode_attn_parts on caches that hold the parent's rows in every child.  Both forms (split + combine, streaming). */
int vis_decode_attn_forked(const void* qkv, const void* cos_t, const void* sin_t, void* k_cache, void* v_cache,
                           const void* step_ptr, void* part_o, void* part_ml, void* out, int Hq, int Hkv, int HD,
                           int cache_tokens, int nsplit, float scale, int batch, long long qkv_bs, long long cache_bs,
                           long long tab_bs, const int* parent, const int* fork_len, vis_stream_t stream);
int vis_decode_attn_parts_forked(const void* part, int ksplit, int slab_rows, const void* bias, const void* sx, const void* sw,
                                 const void* cos_t, const void* sin_t, void* k_cache, void* v_cache, const void* step_ptr,
                                 void* part_o, void* part_ml, void* out, int Hq, int Hkv, int HD, int cache_tokens, int nsplit,
                                 float scale, int batch, long long cache_bs, long long tab_bs, const int* parent,
                                 const int* fork_len, vis_stream_t stream);

/* K10 + K4 + K11 + K10 (single-sequence decode)  the head of a decoder layer as ONE launch:
 *   qkv = W_qkv rmsnorm(x) + b ; attn = attention(rope(q), cache + rope(k), v) ; y = x + W_o attn
 * i.e. vis_gemv_bf16 (norm fused) + vis_decode_attn (split + combine launches) + vis_gemv_bf16 (residual), bit-identical to
 * those four launches (csrc/decode_chain.hip: the stages are workgroup roles of one resident grid that hand their results
 * over as tagged 8-byte granules).  Replaces TF modeling_qwen2_vl.py:501-556 (+ :96-110 input norm) for q_len == 1 with a
 * KV cache.  x [K] bf16 layer input - or, with x_idx != NULL, an [x_rows][K] table whose row *x_idx (a device int, clamped
 * like vis_gather_rows) is the input: the first layer reads the new token's embedding row itself -, Wqkv [(Hq + 2 Hkv) * 128][ldw_qkv], bqkv or NULL, norm_w [K], Wo [K][ldw_o], y [K];
 * tables, caches, step_ptr as vis_decode_attn.
 * ws: vis_decode_chain_ws_bytes(Hq, Hkv, nsplit) bytes and sync: vis_decode_chain_sync_ints() ints, both zeroed once by the
 * caller and owned by one stream; sync[0] counts completed launches, sync[32] is a status word: non-zero after a launch = a
 * bounded wait gave up (results invalid; zero ws and sync before the next launch - until then every further launch on this
 * sync block returns at once without computing: a stranded request costs one wait bound, not one per launch).  The tag of a
 * launch is sync[0] + 1, and 1 after 2^32 - 1 (tag 0 marks a never-written granule): zero ws and sync between requests
 * before sync[0] gets near 2^32.  The packed projection row and the merged
 * attention row live in ws as granules (low 32 bits = two bf16): ws[0 .. (Hq + 2 Hkv) * 64) and the next Hq * 64 words.
 * VIS_ERR_UNSUPPORTED for shapes outside the chained form (HD != 128, Hq / Hkv not in {1, 2, 4, 7, 8}, K or Hq * 128 > 4096,
 * Hq > 64, or more WAITING workgroups - the projection and merge roles plus Hkv attention items per 64 keys of ctx_bound -
 * than the device holds resident minus a margin of 32): the caller then issues the four launches.  ctx_bound: the largest
 * context (cached keys incl. the new one) any launch with these arguments will see (a captured launch is replayed at growing
 * positions), <= 0 = cache_tokens; attention items of splits past the context return at once and need no residency.
 * VIS_ERR_ARG is a caller bug.  ONE chained launch at a time per device: its workgroups wait
 * for each other inside the grid, so launches from two streams at once must be ordered by the caller (an event). */
int vis_decode_chain_sync_ints(void);
long long vis_decode_chain_ws_bytes(int Hq, int Hkv, int nsplit);
/* largest ctx_bound vis_decode_chain accepts for (Hq, Hkv, head_dim 128, hidden K) on the current device; 0 = shape not covered */
int vis_decode_chain_ctx_limit(int Hq, int Hkv, int K);
int vis_decode_chain(const void* x, const void* x_idx, int x_rows, const void* Wqkv, const void* bqkv, const void* norm_w, const void* Wo, void* y,
                     const void* cos_t, const void* sin_t, void* k_cache, void* v_cache, const void* step_ptr,
                     void* ws, void* sync, int Hq, int Hkv, int HD, int K, int ldw_qkv, int ldw_o,
                     int cache_tokens, int nsplit, int ctx_bound, float scale, float eps, vis_stream_t stream);

/* K10 + K12  lm_head of the single-sequence step with the pick's first stage in its epilogue, then the merging launch:
 * logits[N] f32 = W rmsnorm(x); tokens[*step] = cur_token = pick; *step += 1 - the pick vis_gemv_bf16 + vis_argmax_f32 make
 * (same comparison, same Gumbel noise, id 0 when every logit is NaN), one launch fewer.  ws_val / ws_idx: 2048 floats / ints. */
int vis_gemv_bf16_argmax(const void* x, const void* W, const void* norm_w, void* logits, int N, int K, int ldw, float eps,
                         void* ws_val, void* ws_idx, void* tokens, int max_tokens, void* cur_token, void* step_ptr,
                         float inv_temp, unsigned seed, vis_stream_t stream);

/* K12  next-token pick: tokens[*step] = cur_token = argmax(logits) (first index on ties, like
 * torch.argmax), then *step += 1.  inv_temp > 0 samples at temperature 1/inv_temp by Gumbel-max with a
 * counter hash of (seed, *step, index); inv_temp == 0 is greedy (the reference request passes
 * temperature=, src/agents/vlm_inspector.py:108).  NaN logits take no part; a row with no comparable logit (all NaN)
 * picks id 0, never an id outside the vocabulary; step >= max_tokens stores no token but still writes cur_token and
 * advances the step.  ws_val/ws_idx: 256 floats / 256 ints of workspace. */
int vis_argmax_f32(const void* logits, int V, void* ws_val, void* ws_idx, void* tokens, int max_tokens,
                   void* cur_token, void* step_ptr, float inv_temp, unsigned seed, int batch, int ld_logits,
                   vis_stream_t stream);
/* batch > 1: sequence b reads logits + b*ld_logits, writes tokens[b*max_tokens + step[b]], cur_token[b],
 * step_ptr[b]; ws_val / ws_idx need 256 entries per sequence. */

/* Token log-probabilities of the pick vis_argmax_f32 / vis_gemv_bf16_argmax just made (csrc/logprobs.hip).  For sequence
 * b < batch (logits + b * ld_logits, V f32 entries) at pos = step_ptr[b] - 1, if 0 <= pos < max_tokens:
 *   lp[b][pos][0] = logits[tokens[b][pos]] - lse, lse = log(sum exp(logits)) (raw logits: temperature 1, no noise);
 *   lp[b][pos][1 + i] = logits[id_i] - lse and top_ids[b][pos][i] = id_i for i < top_k, descending, ties to the lower index.
 * lp is f32 [batch][max_tokens][21], top_ids int32 [batch][max_tokens][20]; entries past top_k are not written.  A row's results
 * depend on its logits only (the reduction layout is fixed by V).  Own workspace of vis_logprobs_ws_bytes(V, batch) bytes;
 * one launch at a time per workspace.  VIS_ERR_ARG: null pointer, V outside 1..262144, ld_logits < V, batch outside 1..64,
 * top_k outside 0..min(20, V), max_tokens <= 0, ws_bytes too small. */
long long vis_logprobs_ws_bytes(int V, int batch);
int vis_logprobs_f32(const void* logits, int V, int ld_logits, const void* tokens, int max_tokens, const void* step_ptr,
                     int top_k, void* lp, void* top_ids, void* ws, long long ws_bytes, int batch, vis_stream_t stream);

/* JSON mode (csrc/json_mask.hip; the grammar is json_grammar.py's, byte for byte): RFC 8259 text whose top-level value is
 * an object, strictly valid UTF-8, at most 32 open containers and 16 consecutive whitespace bytes.  Run before every pick of
 * a JSON-mode sequence.  For sequence b < batch: state + b * 32 int32 (two slots of 12 words, chosen by the parity of
 * step_ptr[b], and two counters; all zero = a fresh sequence), tokens + b * max_tokens.  The launch folds the tokens
 * picked since the state was last advanced (positions pos .. step_ptr[b] - 1 below max_tokens; none on the first launch
 * after a reset) into the state, then writes allow[b * ld_allow + w] (u64, bit i = token 64 w + i allowed; bits >= V clear).
 * A token is allowed when the grammar accepts all of its bytes (tok_bytes[tok_off[t] .. tok_off[t + 1]), int32 tok_off
 * [V + 1], tok_bytes 4-byte aligned with 4 bytes of padding); tokens without bytes never are; tokens whose tok_flags bit 0
 * is set (EOS) only after the top-level '}'.  Flag bit 1 marks printable ASCII tokens without '"' and '\' (accepted whole
 * inside a string).  A row with no allowed token gets its EOS ids (eos_ids[n_eos]) and the error bit of its state.
 * VIS_ERR_ARG: null pointer, V outside 1..262144, max_tokens <= 0, n_eos outside 1..64, batch outside 1..64,
 * ld_allow < ceil(V / 64), misaligned allow / tok_bytes / state. */
int vis_json_mask(void* state, const void* tokens, int max_tokens, const void* step_ptr, const void* tok_off,
                  const void* tok_bytes, const void* tok_flags, const void* eos_ids, int n_eos, int V, void* allow,
                  int ld_allow, int batch, vis_stream_t stream);
/* Schema-constrained decoding (csrc/schema_mask.hip; json_schema.py compiles the tables and is the reference): vis_json_mask
 * with a byte-level DFA in place of the JSON grammar - same state pitch (32 int32 per sequence: two slots of 12 words chosen
 * by the parity of step_ptr[b], slot words DFA state / error bit / position / anchored, counters at words 24 / 25; all zero =
 * a fresh sequence in the DFA's start state), same folding of the tokens picked since the last launch, same token table,
 * same allow rows, same "no token allowed -> EOS ids + error bit".  The DFA: header int32 [4] = {n_states, n_classes, start,
 * 0}, READ BY THE KERNEL (a captured launch serves whatever schema the buffers hold when it is replayed); trans u16
 * [n_states][n_classes] packed at the front of a buffer of cap_states * cap_classes entries, 65535 = no transition;
 * byte_class u8 [256]; state_flags u8 [cap_states], bit 0 = accepting (EOS ids allowed here only), bit 1 = every printable
 * ASCII byte but '"' and '\' loops (tokens with flag bit 1 are accepted without a walk).  next = trans[s * n_classes +
 * byte_class[byte]].  A header outside the capacities or a state outside the header puts the row in the error state.
 * VIS_ERR_ARG: as vis_json_mask, and null DFA pointer, cap_states outside 1..4096, cap_classes outside 1..256,
 * cap_states * cap_classes * 2 not a multiple of 16, trans not 16-byte aligned, header not 4-byte aligned. */
int vis_schema_mask(void* state, const void* tokens, int max_tokens, const void* step_ptr, const void* tok_off,
                    const void* tok_bytes, const void* tok_flags, const void* eos_ids, int n_eos, int V, void* allow,
                    int ld_allow, const void* header, const void* trans, const void* byte_class, const void* state_flags,
                    int cap_states, int cap_classes, int batch, vis_stream_t stream);
/* vis_argmax_f32 over the allowed ids only: sequence b skips id i unless bit i of allow + b * ld_allow is set.  The
 * comparison (ties to the lower index) and the Gumbel noise are vis_argmax_f32's, so with every bit set the pick is the
 * same bit for bit, and at temperature > 0 it samples the renormalised distribution over the allowed ids.  A row with no
 * allowed id picks id 0.  VIS_ERR_ARG additionally: null allow, ld_allow < ceil(V / 64), allow not 8-byte aligned. */
int vis_argmax_masked_f32(const void* logits, int V, void* ws_val, void* ws_idx, void* tokens, int max_tokens,
                          void* cur_token, void* step_ptr, float inv_temp, unsigned seed, int batch, int ld_logits,
                          const void* allow, int ld_allow, vis_stream_t stream);
/* vis_gemv_bf16_argmax with the pick restricted to the ids allowed by allow[ceil(N / 64)] (every logit is still written). */
int vis_gemv_bf16_argmax_masked(const void* x, const void* W, const void* norm_w, void* logits, int N, int K, int ldw,
                                float eps, void* ws_val, void* ws_idx, void* tokens, int max_tokens, void* cur_token,
                                void* step_ptr, float inv_temp, unsigned seed, const void* allow, vis_stream_t stream);
/* Host only, no launch: the constants with which the shape-specialised bf16 GEMV instances (K = 3584, 18944; single row)
 * split n_pairs row pairs over n_waves (<= 8192) waves without a division: wave w owns pairs [b(w), b(w + 1)),
 * b(w) = q w + ((r w) m >> s), which equals floor(n_pairs w / n_waves) for every w in [0, n_waves] (the launchers check
 * it for every grid they launch; tests/test_gemv_specialised_gpu.py for the grids of its cases). */
int vis_gemv_partition(int n_pairs, int n_waves, int* q, int* r, unsigned* m, int* s);

/* Nucleus (top_p) sampling with per-row seeds (csrc/sampling.hip).  Row b < batch: logits + b * ld_logits (V f32), allowed
 * set A = every id, or (allow non-null) the ids whose bit is set in allow + b * ld_allow (vis_json_mask's rows).  Order A by
 * (logit desc, id asc); w_i = exp((l_i - max) * inv_temp); K = the shortest prefix whose mass >= top_p * sum(w), at least
 * one token.  The pick is the argmax over K of l_i * inv_temp + gumbel_noise(seeds[b], step_ptr[b], i) - vis_argmax_f32's
 * expression and tie rule, so top_p = 1 gives its pick bit for bit for the same row seed.  inv_temp = 0: greedy over A.
 * Effects: tokens[b * max_tokens + step] = pick (step < max_tokens), cur_token[b] = pick, step_ptr[b] += 1; nothing allowed
 * picks id 0.  nkeep (int32 [batch], may be null) = |K| (1 when inv_temp = 0).  seeds: uint32 [batch] in device memory.
 * Masses are summed in fixed point, so a row's K and pick depend only on its own inputs.  Own workspace of
 * vis_sample_ws_bytes(V, batch) bytes (row b uses bytes [b * ws_bytes(V, 1), (b + 1) * ws_bytes(V, 1))); one launch at a
 * time per workspace.  VIS_ERR_ARG: null pointer, V <= 0, batch outside 1..64, ld_logits < V at batch > 1, top_p NaN or
 * outside [0, 1], inv_temp < 0 or NaN, ld_allow < ceil(V / 64) or allow not 8-byte aligned. */
long long vis_sample_ws_bytes(int V, int batch);
int vis_sample_f32(const void* logits, int V, int ld_logits, const void* allow, int ld_allow, float inv_temp, float top_p,
                   const void* seeds, void* tokens, int max_tokens, void* cur_token, void* step_ptr, int batch, void* ws,
                   void* nkeep, vis_stream_t stream);

/* Logit penalties ahead of the pick (csrc/penalty.hip): repetition penalty r (transformers' RepetitionPenaltyLogitsProcessor,
 * over prompt and generated ids), then frequency penalty f and presence penalty q (OpenAI's, over generated ids only):
 *   seen = v in the prompt or c[v] > 0;  y = seen && r != 1 ? (x < 0 ? x * r : x / r) : x;  y -= f * c[v] + q * (c[v] > 0)
 * state: vis_penalty_state_bytes(V, batch) bytes, 16-byte aligned, row b at b * vis_penalty_state_bytes(V, 1); a zeroed row is
 * a fresh sequence (a 16-byte head, then one 16-bit word per id: prompt flag + saturating count of generated occurrences).
 * vis_penalty_prompt marks ids[0 .. n) (int32, device memory) as prompt members of ONE row; ids outside [0, V) are skipped.
 * vis_penalize_f32, one launch per pick: for every row b < batch folds the tokens picked since the row's state was advanced
 * (positions [pos, step[b]) of tokens[b][max_tokens]; none on the first launch after a reset) into the counts and writes
 * out[b][v] for all v; logits are left intact (out != logits).  params: f32 [batch][3] = (r, f, q) in device memory, read at
 * run time.  A launch repeated at the same step changes nothing.  A row's result depends on that row alone.
 * VIS_ERR_ARG: null pointer, V outside 1..262144, batch outside 1..64, max_tokens <= 0, ld_logits / ld_out < V at batch > 1,
 * state not 16-byte aligned, out == logits. */
long long vis_penalty_state_bytes(int V, int batch);
int vis_penalty_prompt(void* state_row, int V, const void* ids, int n, vis_stream_t stream);
int vis_penalize_f32(const void* logits, int V, int ld_logits, void* state, const void* params, const void* tokens,
                     int max_tokens, const void* step_ptr, void* out, int ld_out, int batch, vis_stream_t stream);

/* Logit shaping ahead of the pick (csrc/shape.hip): logit_bias (OpenAI's), then top_k and min_p (transformers'
 * TopKLogitsWarper / MinPLogitsWarper).  Row b < batch, allowed set A = every id, or (allow non-null) the ids whose bit is set
 * in allow + b * ld_allow (vis_json_mask's rows, as vis_sample_f32 takes them):
 *   y[v] = x[v] + bias_vals[b][j] where bias_ids[b][j] == v for some j < nbias[b] (one f32 add; the first such j counts; ids
 *   outside [0, V) are skipped), y[v] = x[v] otherwise;  m = max y over A;
 *   t = the k[b]-th largest y over A when 0 < k[b] < |A| (ties at t all stay), no rank cut otherwise;
 *   v survives when it is in A, y[v] >= t and not (y[v] - m) < delta[b] (f32 subtraction and compare; delta = ln(min_p) /
 *   inv_temp from the host, -inf = off; the row's maximum always survives);
 *   out[b][v] = y[v] for survivors, -inf for every other id (ids outside A included); nkept[b] = the number of survivors.
 * Comparisons are float comparisons (-0.0 == +0.0); inputs are finite.  k int32 [batch], delta f32 [batch], nbias int32
 * [batch] (clamped to 0..300), bias_ids int32 [batch][300], bias_vals f32 [batch][300]: device memory, read at run time, so a
 * captured launch serves any values.  logits are left intact (out != logits).  A row's result depends on that row alone; a
 * repeated launch changes nothing.  ws: vis_shape_ws_bytes(V, batch) bytes, row b receives {f32 t, f32 m, int32 |A|, int32
 * path} (path: 0 no rank cut, 1 cut found by rank counting in LDS, 2 by the radix select; m and |A| are 0 when neither top_k
 * nor min_p is on).  VIS_ERR_ARG and nothing launched: null pointer (allow may be null), V outside 1..262144, batch outside
 * 1..64, ld_logits / ld_out < V at batch > 1, ld_allow < ceil(V / 64) or allow not 8-byte aligned, a pointer not 4-byte
 * aligned, out == logits. */
long long vis_shape_ws_bytes(int V, int batch);
int vis_shape_f32(const void* logits, int V, int ld_logits, const void* allow, int ld_allow, const void* k, const void* delta,
                  const void* nbias, const void* bias_ids, const void* bias_vals, void* out, int ld_out, void* nkept,
                  void* ws, int batch, vis_stream_t stream);

/* Token bans ahead of the pick (csrc/ban.hip; ban.py is the reference): no_repeat_ngram_size (transformers'
 * NoRepeatNGramLogitsProcessor), bad_words (transformers' NoBadWordsLogitsProcessor, vLLM's) and min_tokens (vLLM's).  One
 * launch per pick, after the penalties and ahead of the grammar mask and the shaping.  History of row b < batch: h =
 * prompt_ids[b][0 .. prompt_len[b]) followed by tokens[b][gen_start[b] .. step[b]), L ids, G = step[b] - gen_start[b] of
 * them generated (gen_start = 0: the row holds generated ids only and step counts them, the prompt pass's pick included).
 * Banned:
 *   n = ngram[b] >= 1: h[i+n-1] for every i with i + n - 1 < L and h[i .. i+n-2] == h[L-n+1 .. L-1] (n = 1: every id of h);
 *   word w of m = word_len[w] ids: w[m-1] when m == 1, or when L >= m-1 and h[L-m+1 .. L-1] == w[0 .. m-2] (a match may
 *   straddle the prompt / generated boundary);
 *   every eos_ids[e], e < n_eos, while G < min_tokens[b].
 * out[b][v] = -inf for banned v in [0, V), logits[b][v] bit for bit otherwise; logits are left intact (out != logits); ids of
 * h outside [0, V) are compared like any other and never written.  A row with all three off is copied.  ngram, min_tokens,
 * prompt_len, gen_start int32 [batch], prompt_ids int32 [batch][ld_prompt], words int32 [16][8] (row w = word w), eos_ids
 * int32 [8]: device memory, read at run time - a captured launch serves any values.  word_len: HOST memory, n_words ints;
 * with n_words and n_eos it is a launch argument.  prompt_len is clamped to 0..ld_prompt, step to 0..max_tokens, gen_start
 * to 0..step.  A row's result depends on that row alone; a repeated launch changes nothing.
 * VIS_ERR_ARG and nothing launched: null pointer (word_len may be null at n_words = 0), V outside 1..262144, ld_logits /
 * ld_out < V, batch outside 1..64, max_tokens or ld_prompt <= 0, n_words outside 0..16, a word length outside 1..8, n_eos
 * outside 0..8, a device pointer not 4-byte aligned, out == logits. */
int vis_ban_f32(const void* logits, int V, int ld_logits, const void* prompt_ids, int ld_prompt, const void* prompt_len,
                const void* tokens, int max_tokens, const void* gen_start, const void* step_ptr, const void* ngram,
                const void* min_tokens, const void* words, const int* word_len, int n_words, const void* eos_ids, int n_eos,
                void* out, int ld_out, int batch, vis_stream_t stream);

/* Stop sequences and how a reply ended (csrc/stop_scan.hip; stop.py compiles the tables and is the reference).  One launch
 * AFTER each pick: for every row b < batch folds the tokens picked since the row's last launch (positions [pos, step[b]) of
 * tokens[b][max_tokens]; on the first launch after a reset the one at step[b] - 1) byte by byte - token table as
 * vis_json_mask's - through the Aho-Corasick automaton of the request's stop strings.  state: int32 [batch][8], 16-byte
 * aligned, all zero = a fresh sequence: DFA state, pos, bytes so far, reason (0 open, 1 EOS, 2 stop), tokens kept (EOS:
 * exclusive; stop: through the token that completed the match), cut (byte offset in the generated stream where the match
 * starts; EOS: bytes so far), index of the stop string, anchored.  A row with reason != 0 is never written again; a launch
 * repeated at the same step changes nothing.  The automaton: header int32 [4] = {n_states, n_classes, 0, 0}, READ BY THE
 * KERNEL (a captured launch serves whatever stop set the buffers hold when it is replayed); trans u16 [n_states][n_classes]
 * packed at the front of a buffer of cap_states * cap_classes entries, failure links resolved, bit 15 = the target state
 * ends a stop string; byte_class u8 [256]; hits u8 [cap_states][2] = (length of the longest stop string that is a suffix at
 * the state, its index).  eos_on = 0: tokens flagged EOS are folded as tokens without bytes.  A header outside the
 * capacities switches the walk off; states and classes outside the header are clamped.
 * VIS_ERR_ARG: null pointer, V outside 1..262144, batch outside 1..64, max_tokens <= 0, eos_on not 0 / 1, cap_states outside
 * 1..257, cap_classes outside 1..256, state not 16-byte aligned, tok_bytes / header not 4-byte aligned. */
int vis_stop_scan(void* state, const void* tokens, int max_tokens, const void* step_ptr, const void* tok_off,
                  const void* tok_bytes, const void* tok_flags, int V, const void* header, const void* trans,
                  const void* byte_class, const void* hits, int cap_states, int cap_classes, int eos_on, int batch,
                  vis_stream_t stream);

/* Token-by-token publication of a reply while the decode loop runs (csrc/stream_publish.hip; stream.py is the reference and
 * the reader).  One launch AFTER vis_stop_scan: for every row b < batch whose stop-scan record (stop_state, int32 [batch][8])
 * covers position step[b] - 1 it appends one 16-byte record {token id, safe_bytes, status, cut} at records[b][step[b] - 1]
 * (int32 [batch][capacity][4], one vector store) and then stores count[b] = step[b] with a system-scope release store;
 * start[b] = step[b] - 1 goes out with the row's first record.  records, count and start are HOST memory of
 * vis_host_coherent_alloc (the device addresses).  safe_bytes: bytes of the reply that can no longer be taken back - open
 * row: bytes so far - depth[state] (depth u8 [n_states]: the depth of every automaton state, i.e. the length of the longest
 * suffix of the text that is a prefix of a stop string; a state outside the table counts 0); EOS: the bytes in front of the
 * EOS token; stop: cut, where the match starts.  status: 0 open, 1 EOS, 2 stop.  pub: device int32 [batch], zero = fresh,
 * mirrors count: a launch repeated at the same step changes nothing.  A row that has ended is published once, at the step
 * that ended it, and never again (its count is frozen); nothing published is rewritten.  A position at or beyond capacity or
 * max_tokens is never written.
 * VIS_ERR_ARG and nothing launched: null pointer, stop_state / records not 16-byte aligned, another pointer not 4-byte
 * aligned, batch outside 1..64, max_tokens <= 0, capacity < max_tokens, n_states outside 1..257. */
int vis_stream_publish(const void* stop_state, const void* tokens, int max_tokens, const void* step_ptr, const void* depth,
                       int n_states, void* pub, void* records, int capacity, void* count, void* start, int batch,
                       vis_stream_t stream);

/* Host memory a running kernel stores to coherently: hipHostMalloc with the coherent and mapped flags, zero-filled.
 * *host_ptr: the address the host reads; *dev_ptr: the address kernels are given.  VIS_ERR_ARG: null pointer, bytes outside
 * 1..2^32; VIS_ERR_LAUNCH: the runtime refused.  vis_host_free takes the host address. */
int vis_host_coherent_alloc(void** host_ptr, void** dev_ptr, long long bytes);
int vis_host_free(void* host_ptr);

/* K10 (batched decode), first half.  For up to 64 in-flight sequences the weight matrix is streamed from HBM
 * ONCE per step by <= 256 persistent workgroups (one per CU, 7-stage LDS-DMA ring, stream-K cut of the
 * (128-column tile, K-step) sequence).  part[slot][R][N] (f32), R = 16 / 32 / 64 for B <= 16 / 32 / 64 (one, two or four
 * 16-row MFMA blocks; vis_skinny_finalize uses the same rule): `ksplit` slots, ALL written (unused ones
 * zero-filled), sum over slots = x[B,K] * W[N,K]^T; the slot order is fixed by (N, K) alone, so results are
 * bitwise reproducible.  ksplit <= 0 means vis_gemm_decode_ksplit(N, K) = the slots the geometry needs (<= 16);
 * a smaller value is an argument error.  part == NULL: C is written directly (bf16, or f32 logits when out_f32). */
int vis_gemm_decode_ksplit(int N, int K);
int vis_gemm_decode_bf16(const void* x, const void* W, void* part, void* C, int B, int N, int K, int ldx, int ldw,
                         int ldc, int ksplit, int out_f32, vis_stream_t stream);

/* K10 (batched decode), second half: one workgroup per sequence sums the K-slices in a fixed order (bitwise
 * reproducible), applies bias / residual or SwiGLU (16-column interleaved gate/up, N/2 outputs) -> y, and when
 * norm_w != NULL also writes yn = bf16(bf16(y * rsqrt(mean(y^2) + eps)) * norm_w) - the RMSNorm'd input of the
 * NEXT projection (TF modeling_qwen2_vl.py:96-110,:459-466,:598-624). */
int vis_skinny_finalize(const void* part, int ksplit, const void* bias, const void* R, const void* norm_w, void* y,
                        void* yn, int B, int N, int ldr, int ldy, int ldyn, int swiglu, float eps,
                        vis_stream_t stream);

/* Row f3: bicubic resample of the decoded RGB frame, bit-exact with Pillow's 8-bit ImagingResample (the
 * resampler behind the HF Qwen2-VL processor's resize(resample=BICUBIC),
 * TF:models/qwen2_vl/image_processing_qwen2_vl.py:62-89,:165-198; replaces the host-side PIL call of the service
 * half of reference step a3, src/agents/vlm_inspector.py:46-88).  src u8 [in_h][in_w][3] -> dst u8
 * [out_h][out_w][3], tmp u8 [in_h][out_w][3].  kx int32 [out_w][ksx] / bx int32 [out_w][2] = {first column,
 * taps}: fixed-point (22 fractional bits) filter rows of the horizontal pass; ky/by the same for the vertical pass
 * (built on the host by image_processing.resample_coeffs).  All pointers are device pointers. */
int vis_resize_rgb_u8(const void* src, void* tmp, void* dst, int in_h, int in_w, int out_h, int out_w,
                      const void* kx, const void* bx, int ksx, const void* ky, const void* by, int ksy, void* stream);

/* Service-side JPEG decode, GPU half (csrc/jpeg.hip; host half: include/vis_jpeg_host.h).  Replaces the libjpeg decode
 * of the data-URI image the reference's agents send (src/agents/vlm_inspector.py:46-88 writes it; the service reads it).
 * coeffs: int16 [blocks][64] quantised DCT coefficients in natural order, component planes back to back (Y, Cb, Cr),
 * blocks row-major; qt: int32 [3][64]; planes: workspace of blocks * 64 bytes; rgb: uint8 [height][width][3].
 * hs / vs: luma sampling factors (1x1, 2x1 or 2x2; chroma is 1x1); bw / bh: blocks per row / column of the luma and the
 * chroma planes; dw_c / dh_c: real chroma size in samples.  Integer arithmetic throughout: the result equals
 * libjpeg-turbo's default decoder (islow IDCT, fancy upsampling) bit for bit. */
int vis_jpeg_to_rgb(const void* coeffs, const void* qt, void* planes, void* rgb, int width, int height, int ncomp,
                    int hs, int vs, int bw_y, int bh_y, int bw_c, int bh_c, int dw_c, int dh_c, vis_stream_t stream);

/* K1 (front)  resized RGB u8 frame [H][W][3] -> normalised bf16 patch rows
 * out[row0 + p][ld_out] in the merge-group order of
 * TF image_processing_pil_qwen2_vl.py:156-190; mean/stdv are HOST pointers to 3 floats. */
int vis_patchify_u8(const void* img, void* out, int H, int W, int ld_out, int row0, const float* mean,
                    const float* stdv, vis_stream_t stream);

/* K12  out[i][:] = table[ids[i]][:] (embedding lookup, ids int32 on device). */
int vis_gather_rows(const void* table, const void* ids, void* out, int n, int D, int n_table,
                    vis_stream_t stream);

/* K12  dst[idx[i]][:] = src[i][:] (image-token scatter, TF modeling_qwen2_vl.py:1144-1200). */
int vis_scatter_rows(const void* src, const void* idx, void* dst, int n, int D, int n_dst,
                     vis_stream_t stream);

/* K2, split-K form for long-K problems whose 256x256 tile count cannot fill the chip (LLM down projection: 126 tiles,
 * K = 18944): `ksplit` (2..8) K-slices run as independent tiles, f32 partials go to `work` (ksplit*M*N floats), a
 * second launch sums them in a fixed order and applies bias / act (0..2) / residual.  N % 8 == 0, no SwiGLU. */
int vis_gemm_bf16_splitk(const void* A, const void* W, const void* bias, const void* R, void* C, void* work, int M, int N,
                         int K, int lda, int ldw, int ldc, int ldr, int act, int ksplit, vis_stream_t stream);
/* The K-sliced tiles of vis_gemm_bf16_splitk alone: work[ksplit][M][N] f32 partial sums of A W^T (no finalisation). */
int vis_gemm_bf16_splitk_part(const void* A, const void* W, void* work, int M, int N, int K, int lda, int ldw,
                              int ksplit, vis_stream_t stream);
/* Their finalisation fused with the NEXT norm of the block (K3 / K5; the row owner exists here):
 * x = bf16(sum_s part[s] + bias + R); y = RMSNorm(x) * norm_w (norm_b == NULL) or LayerNorm(x) (norm_b != NULL), with
 * the statistics of the rounded x - bit-identical to vis_gemm_bf16_splitk followed by vis_rmsnorm_bf16 /
 * vis_layernorm_bf16.  y == NULL: finalisation only.  N <= 5120, N % 8 == 0. */
int vis_splitk_finalize_norm(const void* part, int ksplit, const void* bias, const void* R, void* x,
                             const void* norm_w, const void* norm_b, void* y, int M, int N, int ldr, int ldx, int ldy,
                             float eps, vis_stream_t stream);

/* BASELINE configs[4] slice - fp8 weights for the HBM-bound decode projections ("W8A16"):
 * y = act((Wq x) * scale + bias) + R with Wq OCP e4m3 bytes [N][ldw] and a per-output-row f32 scale; x bf16 with the
 * same fused RMSNorm prologue / bias / residual / SwiGLU (16-row interleaved gate/up) / f32-output options as
 * vis_gemv_bf16.  Halves the bytes per generated token (14.14 GB -> 7.07 GB at 7B). */
int vis_gemv_fp8w(const void* x, const void* Wq, const void* scale, const void* bias, const void* R,
                  const void* norm_w, void* y, int N, int K, int ldw, int act, int out_f32, float eps,
                  vis_stream_t stream);

/* K10 (batched decode), round 5: projection + split-K reduction + row-wise epilogue in ONE launch (csrc/decode_stream.hip);
 * replaces vis_gemm_decode_* + vis_skinny_finalize* in the engines (those stay exported).  Same persistent stream-K ring;
 * a tile cut between workgroups is summed, in fixed segment order, by whichever of them takes the tile's last ticket
 * (nobody waits), then finished there:
 *   VIS_DP_PLAIN       C[b][n] = (x W^T)[b][n] * rs[b] + bias[n]         bf16, or f32 when out_f32 (q/k/v, lm_head)
 *   VIS_DP_SWIGLU      C[b][o] = silu(g * rs[b]) * (u * rs[b])           16-row interleaved gate/up weight, N / 2 outputs
 *   VIS_DP_RESID_NORMW C = y = bf16(x W^T + R), Cw = bf16(y * nw[n]), ssq_out[n / 32][b] = sum over the 32-column unit of y^2
 * The RMSNorm in front of a projection (TF modeling_qwen2_vl.py:96-110) is applied in two exact halves: the PRODUCER of the
 * row multiplies by the norm weight (Cw, a per-column factor), the CONSUMER by rs[b] = rsqrt(sum_t ssq_in[t][b] / norm_dim +
 * eps) (a per-row factor that commutes with the projection); ssq_in == NULL means rs = 1.  ssq buffers: [columns / 32][64]
 * f32 (tiles_in = norm_dim / 32 <= 128 units).
 * ws: vis_decode_proj_ws_bytes(B, N, K, fp8) bytes, 256-byte aligned, zeroed once (the kernel leaves it reusable), one
 * launch at a time per workspace.  A row's result depends on that row alone (bitwise slot / batch-size invariance).
 * Cq / Cqs (SWIGLU, RESID_NORMW; may be NULL): the row the next projection consumes (act, or y * nw) as MX blocks: OCP
 * e4m3 bytes [B][ldcq] + one E8M0 scale byte per 32 columns [B][ldcqs] (the smallest power of two with block maximum /
 * scale <= 448).  vis_decode_proj_fp8 (BASELINE configs[4]): A given as such blocks (Aq, As), Wq e4m3 [N][ldw] with
 * per-output-row f32 scales sw[N], on v_mfma_scale_f32_16x16x128_f8f6f4 with the block scale in the instruction's scale
 * operand; K % 128 == 0.  vis_decode_prep_rows: head of a step - x[b] = table[ids[b]] (clamped), xw = bf16(x * nw), the
 * MX copy of xw (xq / xqs, may be NULL) and ssq[n / 32][b]; H % 128 == 0. */
#define VIS_DP_PLAIN 0
#define VIS_DP_SWIGLU 1
#define VIS_DP_RESID_NORMW 2
long long vis_decode_proj_ws_bytes(int B, int N, int K, int fp8);
int vis_decode_proj_bf16(const void* A, const void* W, void* ws, void* C, void* Cw, void* Cq, void* Cqs,
                         const void* bias, const void* R, const void* nw, const void* ssq_in, void* ssq_out,
                         int B, int N, int K, int lda, int ldw, int ldc, int ldr, int ldcq, int ldcqs, int mode,
                         int out_f32, int tiles_in, int norm_dim, float eps, vis_stream_t stream);
int vis_decode_proj_fp8(const void* Aq, const void* As, const void* Wq, const void* sw, void* ws, void* C,
                        void* Cw, void* Cq, void* Cqs, const void* bias, const void* R, const void* nw,
                        const void* ssq_in, void* ssq_out, int B, int N, int K, int ldaq, int ldas, int ldw,
                        int ldc, int ldr, int ldcq, int ldcqs, int mode, int out_f32, int tiles_in,
                        int norm_dim, float eps, vis_stream_t stream);
/* Column-parallel form of the same projection (csrc/decode_colpar.hip): every workgroup owns whole output columns - floor or
 * ceil((N / 32) / workgroups) units of 32 columns, at most five, min(256, N / 32) workgroups - and the entire K, so nothing is
 * reduced across workgroups: no workspace, no tickets, the epilogue runs on registers.  Each workgroup streams all of x
 * (rows x K, from L2) next to its weight rows (from HBM): the form for projections whose x is small next to the weights a
 * workgroup owns (everything but the long-K down projection at many sequences).  Arguments, epilogue modes and per-row
 * results as vis_decode_proj_* (a row's sum runs over the K-steps in ascending order in both forms; tiles the stream-K form
 * does not cut are bit-identical).  vis_decode_proj_colpar_covers: 1 when the form covers (N, mode, MX output wanted) - N %
 * 32 == 0, N <= 40960, not SwiGLU with an MX output (an act block of 32 columns spans two units); otherwise the entry
 * points return VIS_ERR_UNSUPPORTED and the caller uses vis_decode_proj_*. */
int vis_decode_proj_colpar_covers(int N, int mode, int mx_out);
int vis_decode_proj_colpar_bf16(const void* A, const void* W, void* C, void* Cw, void* Cq, void* Cqs, const void* bias,
                                const void* R, const void* nw, const void* ssq_in, void* ssq_out, int B, int N, int K,
                                int lda, int ldw, int ldc, int ldr, int ldcq, int ldcqs, int mode, int out_f32,
                                int tiles_in, int norm_dim, float eps, vis_stream_t stream);
int vis_decode_proj_colpar_fp8(const void* Aq, const void* As, const void* Wq, const void* sw, void* C, void* Cw,
                               void* Cq, void* Cqs, const void* bias, const void* R, const void* nw,
                               const void* ssq_in, void* ssq_out, int B, int N, int K, int ldaq, int ldas, int ldw,
                               int ldc, int ldr, int ldcq, int ldcqs, int mode, int out_f32, int tiles_in,
                               int norm_dim, float eps, vis_stream_t stream);
int vis_decode_prep_rows(const void* table, const void* ids, const void* nw, void* x, void* xw, void* xq,
                         void* xqs, void* ssq, int B, int table_rows, int H, int ldx, int ldq, int ldqs,
                         vis_stream_t stream);

/* K10 for a handful of in-flight sequences (1 <= B <= 4): vis_gemv_bf16 / vis_gemv_fp8w over B input rows
 * (x [B][ldx], y [B][ldy], R [B][ldr]; bias and norm_w shared).  The weights are streamed ONCE for all rows, each row's
 * arithmetic is the single-row kernel's (bit-identical results), and - unlike vis_gemm_decode_* + vis_skinny_finalize* -
 * there is no partial buffer and no finalisation launch.  B * K * 2 bytes of LDS (<= 152 KiB). */
int vis_gemv_bf16_rows(const void* x, const void* W, const void* bias, const void* R, const void* norm_w, void* y,
                       int B, int N, int K, int ldw, int ldx, int ldy, int ldr, int act, int out_f32, float eps,
                       vis_stream_t stream);
int vis_gemv_fp8w_rows(const void* x, const void* Wq, const void* scale, const void* bias, const void* R,
                       const void* norm_w, void* y, int B, int N, int K, int ldw, int ldx, int ldy, int ldr, int act,
                       int out_f32, float eps, vis_stream_t stream);

/* Decode projections on OCP Microscaling FP4 weights ("W4A16", csrc/decode_fp4.hip):
 * y = act(sum_k deq(Wq, Ws)[n][k] * x[k] + bias) + R, f32 accumulation, x bf16 with the options of vis_gemv_fp8w
 * (fused RMSNorm prologue, bias / residual, SwiGLU on the 16-row interleaved gate/up with N % 64 == 0, bf16 or f32 y).
 * Wq uint8 [N][ldq]: byte j of a row holds the E2M1 codes (sign << 3 | exp << 1 | man: +-{0, .5, 1, 1.5, 2, 3, 4, 6})
 * of element 2j in its low and 2j+1 in its high nibble; ldq >= K/2, ldq % 16 == 0.  Ws uint8 [N][lds], lds >= K/32: one
 * E8M0 byte b per 32 consecutive K-elements of a row, scale 2^(b-127), b in 3..250 (every product then is a normal bf16);
 * no second-level scale.  K % 32 == 0, K * 2 <= 60 KiB.  A quarter of the bf16 bytes per generated token plus 1/16 for
 * the scales (14.14 GB -> 3.76 GB at 7B).
 * _rows: 1 <= B <= 4 input rows as vis_gemv_fp8w_rows (x [B][ldx], y [B][ldy], R [B][ldr]); every row bit-identical to
 * the single-row call. */
int vis_gemv_mxfp4w(const void* x, const void* Wq, const void* Ws, const void* bias, const void* R,
                    const void* norm_w, void* y, int N, int K, int ldq, int lds, int act, int out_f32, float eps,
                    vis_stream_t stream);
int vis_gemv_mxfp4w_rows(const void* x, const void* Wq, const void* Ws, const void* bias, const void* R,
                         const void* norm_w, void* y, int B, int N, int K, int ldq, int lds, int ldx, int ldy, int ldr,
                         int act, int out_f32, float eps, vis_stream_t stream);

/* Batched decode projection on the same MXFP4 weights (csrc/decode_fp4_batched.hip): vis_gemm_decode_bf16 on
 * deq(Wq, Ws) with the codes and scales streamed ONCE for 5 <= B <= 64 sequences (persistent stream-K workgroups, LDS-DMA
 * ring, codes de-quantised in registers into exact bf16 MFMA fragments, f32 accumulation).  x bf16 [B][ldx], ldx % 8 == 0,
 * ldx >= K; Wq / Ws as above (padded ldq / lds allowed); K % 64 == 0, N % 4 == 0; x, Wq, part and C 16-byte aligned.
 * Output contract of vis_gemm_decode_bf16: part[slot][R][N] f32 with R = 16 / 32 / 64 for B <= 16 / 32 / 64, `ksplit`
 * slots ALL written (unused ones zero-filled) whose sum is the projection; ksplit <= 0 means
 * vis_gemm_decode_mxfp4_ksplit(N, K) (<= 16, fixed by (N, K) alone; 0 for N <= 0 or K < 64), a smaller value is an
 * argument error, a larger one (<= 16) only adds zero slots.  part == NULL: C [B][ldc] is written directly (bf16, or
 * f32 when out_f32; ldc % 4 == 0, ldc >= N).  The K order and the stream-K cut do not depend on B or on a row's position:
 * a row's result is bit-identical in every batch of 5..64.  It is NOT the summation order of vis_gemv_mxfp4w[_rows].
 * Anything else returns VIS_ERR_ARG and launches nothing. */
int vis_gemm_decode_mxfp4_ksplit(int N, int K);
int vis_gemm_decode_mxfp4(const void* x, const void* Wq, const void* Ws, void* part, void* C, int B, int N, int K,
                          int ldx, int ldq, int lds, int ldc, int ksplit, int out_f32, vis_stream_t stream);

/* BASELINE configs[4]: GEMM on the CDNA4 block-scaled fp8 MFMA (v_mfma_scale_f32_16x16x128_f8f6f4, unit block scales).
 * C[M, N(/2)] = act((Aq Wq^T) * sa[m] * sw[n] + bias) + R with Aq [M][lda] / Wq [N][ldw] OCP e4m3 bytes, per-row f32
 * scales sa [M] (per token, vis_quant_rows_fp8) and sw [N] (per output channel); act as vis_gemm_bf16; K % 128 == 0.
 * work != NULL: split-K over `ksplit` (2..8) K-slices with f32 partials in work (ksplit*M*N floats) and a fixed-order
 * finalisation (long-K problems with too few 256x256 tiles; N % 8 == 0, no SwiGLU); work == NULL: single pass. */
int vis_gemm_fp8(const void* Aq, const void* sa, const void* Wq, const void* sw, const void* bias, const void* R,
                 void* C, void* work, int ksplit, int M, int N, int K, int lda, int ldw, int ldc, int ldr, int act,
                 vis_stream_t stream);

/* Host-only (no HIP call, callable without a GPU): what vis_gemm_bf16 / vis_gemm_fp8 would launch for this problem,
 * honouring the VIS_GEMM_* A/B variables exactly as the launchers do (both launch FROM this plan).  aligned16: C and R
 * (if any) are 16-byte aligned; split: a split-K call of vis_gemm_fp8 (work != NULL).  Writes plan[0] = launches,
 * plan[1] = LDS-staged "wide" epilogue (else direct), plan[2] = non-temporal C stores, then per launch five ints
 * {kernel id, first W row, W rows, tiles_m, tiles_n}.  Kernel ids, the same in both queries: 1 = 128x128, 7 = 256x256 ping-pong,
 * 8 = 128x256 ping-pong half-tiles (bf16 only); they are also the values VIS_GEMM_TILE (1, 7, 8) and VIS_GEMM8_TILE
 * (1, 7) accept.  Returns the number of launches (<= 4), or 0 for arguments the launcher rejects by shape, when
 * plan_ints < 3 + 5 * launches, or when that variable holds any other non-zero value (the launchers then return
 * VIS_ERR_ARG).
 * The queries see no pointers: what the launchers reject by pointer (null, misaligned operands) or by the presence of a
 * bias (vis_gemm_fp8 takes none with SwiGLU) still gets a plan. */
int vis_gemm_bf16_plan(int M, int N, int K, int ldc, int ldr, int act, int has_residual, int aligned16, int* plan,
                       int plan_ints);
int vis_gemm_fp8_plan(int M, int N, int K, int ldc, int ldr, int act, int has_residual, int aligned16, int split,
                      int* plan, int plan_ints);

/* Per-row dynamic quantisation of bf16 activations to e4m3: scale[m] = amax(row)/448, q = rne(x * (1/scale)); with
 * norm_w != NULL the row is normalised first (K <= 4096): RMSNorm when norm_b == NULL, LayerNorm otherwise - the
 * same bf16 values vis_rmsnorm_bf16 / vis_layernorm_bf16 write. */
int vis_quant_rows_fp8(const void* x, const void* norm_w, const void* norm_b, void* q, void* scale, int rows, int K,
                       int ldx, int ldq, float eps, vis_stream_t stream);

/* BASELINE configs[4], batched decode: fp8 forms of vis_gemm_decode_bf16 / vis_skinny_finalize.
 * vis_gemm_decode_fp8: xq [B][ldx] / Wq [N][ldw] OCP e4m3 bytes (K % 128 == 0) on the block-scaled fp8 MFMA, same
 * persistent stream-K ring; partials (part != NULL) are RAW sums, the direct form (part == NULL) applies sx[b]*sw[n].
 * vis_skinny_finalize_fp8: sums the partial slots, scales by sx[b]*sw[n], then bias / residual / SwiGLU / next
 * RMSNorm as vis_skinny_finalize; yq != NULL additionally writes the row the NEXT projection consumes (yn if normed,
 * else y) as e4m3 bytes with its per-row scale yq_scale[b] = amax/448 (the activation quantiser, fused). */
int vis_gemm_decode_fp8_ksplit(int N, int K);
int vis_gemm_decode_fp8(const void* xq, const void* sx, const void* Wq, const void* sw, void* part, void* C, int B,
                        int N, int K, int ldx, int ldw, int ldc, int ksplit, int out_f32, vis_stream_t stream);
int vis_skinny_finalize_fp8(const void* part, int ksplit, const void* sx, const void* sw, const void* bias,
                            const void* R, const void* norm_w, void* y, void* yn, void* yq, void* yq_scale, int B,
                            int N, int ldr, int ldy, int ldyn, int ldyq, int swiglu, float eps, vis_stream_t stream);

/* ---- Lossless n-gram speculative decoding of one greedy sequence (csrc/spec.hip, spec.py) ----
 * A step runs R = 1 + k rows (1 <= R <= 4: the current token and up to k drafted ones) through vis_gemv_*_rows, then:
 *
 * vis_decode_attn_draft: vis_decode_attn for the `rows` rows of ONE sequence.  Row r of qkv [rows][qkv_ld] (packed
 * projection rows, qkv_ld >= (Hq + 2 Hkv) * 128, a multiple of 8) sits at position *step_ptr + r: rope row, cache row and
 * keys [0, *step_ptr + r] follow from it; the rows are causal among themselves.  Caches [Hkv][cache_tokens][128], tables
 * [cache_tokens][128], workspaces part_o [rows][Hq][nsplit][128] / part_ml [rows][Hq][nsplit][2] f32, out [rows][Hq*128].
 * Three launches (append every row, attend, combine) with vis_decode_attn's split plan and key order: output row r and
 * the cache are bit-identical to `rows` successive vis_decode_attn launches at advancing steps.  A row at a position
 * >= cache_tokens reads and writes nothing (its output row keeps what it held).  *step_ptr is not changed. */
int vis_decode_attn_draft(const void* qkv, const void* cos_t, const void* sin_t, void* k_cache, void* v_cache,
                          const void* step_ptr, void* part_o, void* part_ml, void* out, int Hq, int Hkv, int HD,
                          int cache_tokens, int nsplit, float scale, int rows, long long qkv_ld, vis_stream_t stream);

/* vis_decode_cross_attn_draft (csrc/cross_attn.hip): vis_decode_cross_attn (below) for the `rows` (1..4) rows of ONE sequence's
 * speculative step.
 * Row r's q is q + r * q_ld (q_ld >= Hq * 128, a multiple of 8: the leading columns of a wider projection row may be passed);
 * all rows attend the same static keys [0, *nkeys_m1 + 1) - one count, read from device memory and clamped into
 * [.., key_tokens).  One workgroup per (kv head, split of 64 keys) loads the split's K / V once and serves every row: row r's
 * normalised heads take columns r G .. r G + G - 1 of the score MFMA's 16, hence rows * G <= 16 (G = Hq / Hkv; G = 7, 8: rows
 * <= 2).  Workspaces part_o [rows][Hq][nsplit][128] / part_ml [rows][Hq][nsplit][2] f32, out [rows][Hq*128].  Output row r is
 * bit-identical to vis_decode_cross_attn on q row r alone and does not depend on `rows` or on the other rows.  Argument checks:
 * vis_decode_cross_attn's, rows, q_ld and rows * G <= 16; VIS_ERR_ARG launches nothing. */
int vis_decode_cross_attn_draft(const void* q, const void* q_norm_w, const void* k, const void* v, const void* nkeys_m1,
                                void* part_o, void* part_ml, void* out, int Hq, int Hkv, int HD, int key_tokens, int nsplit,
                                float scale, float eps, int rows, long long q_ld, vis_stream_t stream);
/* The same over the fp8 copies of the keys / values (vis_decode_cross_attn_fp8's operands and checks; csrc/cross_attn.hip):
 * output row r is bit-identical to vis_decode_cross_attn_fp8 on q row r alone. */
int vis_decode_cross_attn_fp8_draft(const void* q, const void* q_norm_w, const void* k_codes, const void* k_scale,
                                    const void* v_codes, const void* v_scale, const void* nkeys_m1, void* part_o,
                                    void* part_ml, void* out, int Hq, int Hkv, int HD, int key_tokens, int nsplit,
                                    float scale, float eps, int rows, long long q_ld, vis_stream_t stream);

/* vis_spec_accept: p_r = the greedy pick of logits row r ([rows][ld_logits] f32; vis_argmax_f32's comparison: ties to the
 * lowest id, a row without a comparable logit picks 0); d = *n_draft clamped to 0..rows-1; a = the number of leading
 * r < d with draft[r] == p_r, clamped so that *step_ptr + a <= *limit (the last index of `tokens` the request may
 * write; also clamped to max_tokens - 1).  Writes tokens[*step_ptr + r] = p_r for r = 0..a, *cur_token = p_a,
 * *step_ptr += a + 1 and adds (1, d, a) to counters[0..2] (steps, proposed, accepted).  With *step_ptr > *limit on
 * entry nothing is written at all.  ws_val / ws_idx: 256 entries per row.  Two launches. */
int vis_spec_accept(const void* logits, int V, int ld_logits, int rows, const void* draft, const void* n_draft,
                    const void* limit, void* ws_val, void* ws_idx, void* tokens, int max_tokens, void* cur_token,
                    void* step_ptr, void* counters, vis_stream_t stream);

/* vis_spec_accept_sampled: vis_spec_accept for a sampled request.  params: 8 bytes of device memory {float inv_temp,
 * uint32 seed}, read when the launch runs (a captured step serves every temperature and seed).  p_r = the Gumbel-max pick
 * of row r at hash counter s = (unsigned)(*step_ptr + r): argmax_i of logits[r][i] * inv_temp + gumbel_noise(seed, s, i),
 * the expression and tie rule of vis_argmax_f32 (a larger value wins, an equal one goes to the lower id, NaN is never
 * picked, a row without a comparable value picks 0) - bit for bit the token vis_argmax_f32 (batch 1) stores for that row
 * with *step_ptr = s and that seed.  An inv_temp that is not > 0 gives vis_spec_accept's picks.  Everything behind the
 * picks - d, a, limit, tokens, *cur_token, *step_ptr, counters - is vis_spec_accept's.  Argument checks: vis_spec_accept's,
 * and params non-null and 4-byte aligned; VIS_ERR_ARG launches nothing.  Two launches. */
int vis_spec_accept_sampled(const void* logits, int V, int ld_logits, int rows, const void* draft, const void* n_draft,
                            const void* limit, void* ws_val, void* ws_idx, void* tokens, int max_tokens, void* cur_token,
                            void* step_ptr, void* counters, const void* params, vis_stream_t stream);

/* vis_spec_accept_masked (csrc/spec.hip): vis_spec_accept / vis_spec_accept_sampled with row r's pick restricted to the ids
 * whose bit is set in allow + r * ld_allow (u64 words, vis_schema_mask_rows' rows).  params null: the greedy pick; else
 * vis_spec_accept_sampled's 8 bytes.  p_r is bit for bit the token vis_argmax_masked_f32 (batch 1) stores for that row with
 * *step_ptr = step + r (and that inverse temperature and seed); a row without an allowed id picks 0.  Everything behind the
 * picks is vis_spec_accept's.  Argument checks: vis_spec_accept's, and allow non-null and 8-byte aligned, ld_allow >=
 * ceil(V / 64), params 4-byte aligned; VIS_ERR_ARG launches nothing.  Two launches. */
int vis_spec_accept_masked(const void* logits, int V, int ld_logits, int rows, const void* draft, const void* n_draft,
                           const void* limit, void* ws_val, void* ws_idx, void* tokens, int max_tokens, void* cur_token,
                           void* step_ptr, void* counters, const void* params, const void* allow, int ld_allow,
                           vis_stream_t stream);

/* vis_spec_draft: prompt lookup over the history h = prompt_ids[0 .. *prompt_len) followed by tokens[*gen_start ..
 * *step_ptr) (vis_ban_f32's reading), length L.  For m = lookup_max down to lookup_min (1 <= min <= max <= 8) with
 * L > m: the LATEST j < L - m with h[j .. j+m) == h[L-m .. L); the first m with a match writes draft[0 .. d) =
 * h[j+m .. j+m+d), d = min(k, L - j - m) (1 <= k <= 3; ids clamped into [0, vocab)), and *n_draft = d.  No match:
 * *n_draft = 0, draft untouched.  One workgroup, no host round trip.  spec.propose() is the definition. */
int vis_spec_draft(const void* prompt_ids, int ld_prompt, const void* prompt_len, const void* tokens, int max_tokens,
                   const void* gen_start, const void* step_ptr, int k, int lookup_max, int lookup_min, int vocab,
                   void* draft, void* n_draft, vis_stream_t stream);

/* vis_spec_draft_pred: the drafter of a request that came with a prediction (OpenAI's Predicted Outputs): exactly one
 * spec.propose_pred() call on device memory.  The arguments of vis_spec_draft, plus pred_ids [ld_pred] with *pred_len of
 * them valid (clamped to 0..ld_pred) and state, 7 ints (spec.PredState): cursor (index into pred_ids of the id expected
 * next, -1 = lost), last (the cursor before it was lost), seen (reply tokens consumed), src / n_out (source - 0 none,
 * 1 prompt lookup, 2 prediction - and count of the drafts of the previous call), accepted, rejected.  The reply is
 * tokens[*gen_start .. *step_ptr).  The new reply tokens settle the previous drafts (accepted += min(new - 1, n_out),
 * rejected += the rest, prediction-sourced drafts only) and move the cursor; a lost cursor is looked for again: for m =
 * lookup_max down to lookup_min, e in [m, *pred_len) with pred_ids[e-m .. e) == the reply's last m ids, the smallest
 * e >= last, else the largest e < last.  Draft: pred_ids[cursor .. cursor + min(k, *pred_len - cursor)) while the cursor
 * stands inside the prediction, else vis_spec_draft's lookup over prompt + reply.  Ids clamped into [0, vocab).  One
 * workgroup, one launch, no host round trip: a captured step serves any prediction up to ld_pred ids. */
int vis_spec_draft_pred(const void* prompt_ids, int ld_prompt, const void* prompt_len, const void* tokens, int max_tokens,
                        const void* gen_start, const void* step_ptr, int k, int lookup_max, int lookup_min, int vocab,
                        const void* pred_ids, int ld_pred, const void* pred_len, void* state, void* draft, void* n_draft,
                        vis_stream_t stream);

/* ---- The speculative step of a BATCH (csrc/spec.hip, spec_batch.py): `batch` in-flight sequences of `rows` rows each run
 * as batch * rows <= 64 rows of the stream-K projection; packed row b * rows + r is row r of sequence b.
 *
 * vis_decode_attn_streams: host only, no launch - 1 when vis_decode_attn would take the streaming form for `batch` sequences
 * of Hkv kv heads (Hkv * batch >= 128, or VIS_DECODE_ATTN_STREAM says so), else 0.
 *
 * vis_decode_attn_draft_batch: vis_decode_attn_draft for `batch` sequences.  Row (b, r) of qkv [batch * rows][qkv_ld] sits at
 * position step_ptr[b] + r of sequence b: rope row, cache row and keys [0, step_ptr[b] + r] come from sequence b's tables
 * (cos_t / sin_t + b * tab_bs) and caches (+ b * cache_bs, element strides as in vis_decode_attn); the rows of one sequence
 * are causal among themselves.  Workspaces part_o [batch * rows][Hq][nsplit][128] / part_ml [..][2] f32, out
 * [batch * rows][Hq*128].  Three launches (append every row of every sequence, attend, combine) with the split plan, key
 * order and combine of vis_decode_attn's split form: output row (b, r) and every cache are bit-identical to `rows` successive
 * vis_decode_attn(batch) launches at advancing steps.  A row at a position >= cache_tokens reads and writes nothing;
 * step_ptr is not changed.  Split form only: where vis_decode_attn_streams(Hkv, batch) holds - the plain step of these
 * sequences would stream - VIS_ERR_UNSUPPORTED and nothing is launched.  VIS_ERR_ARG: vis_decode_attn_draft's checks, batch
 * outside 1..64, batch * rows > 64, cache_bs < Hkv * cache_tokens * 128 or no multiple of 8, tab_bs < 0. */
int vis_decode_attn_streams(int Hkv, int batch);
int vis_decode_attn_draft_batch(const void* qkv, const void* cos_t, const void* sin_t, void* k_cache, void* v_cache,
                                const void* step_ptr, void* part_o, void* part_ml, void* out, int Hq, int Hkv, int HD,
                                int cache_tokens, int nsplit, float scale, int rows, int batch, long long qkv_ld,
                                long long cache_bs, long long tab_bs, vis_stream_t stream);

/* vis_spec_gather_batch: the input rows of the step - out[b * rows + r][0 .. D) = table[id][0 .. D) (bf16, D % 8 == 0) with
 * id = cur_token[b] for r = 0 and draft[b][r - 1] behind it, clamped into [0, n_table) (vis_gather_rows' copy).  draft is
 * [batch][3].  One launch. */
int vis_spec_gather_batch(const void* table, const void* cur_token, const void* draft, void* out, int rows, int batch, int D,
                          int n_table, vis_stream_t stream);

/* vis_spec_accept_batch: vis_spec_accept (params null) or vis_spec_accept_sampled per sequence.  logits
 * [batch * rows][ld_logits] f32, draft [batch][3], n_draft / limit / cur_token / step_ptr [batch], tokens
 * [batch][max_tokens], counters [batch][3], params [batch][2] ({float inv_temp, uint32 seed} of sequence b) or null, ws_val
 * / ws_idx 256 entries per row.  Row (b, r)'s pick is the greedy pick, or the Gumbel-max pick at hash counter
 * step_ptr[b] + r with sequence b's inverse temperature and seed; every output of sequence b is bit for bit what the
 * single-sequence entry writes given b's rows and state alone.  Argument checks: vis_spec_accept's, batch outside 1..64,
 * batch * rows > 64; VIS_ERR_ARG launches nothing.  Two launches. */
int vis_spec_accept_batch(const void* logits, int V, int ld_logits, int rows, int batch, const void* draft,
                          const void* n_draft, const void* limit, void* ws_val, void* ws_idx, void* tokens, int max_tokens,
                          void* cur_token, void* step_ptr, void* counters, const void* params, vis_stream_t stream);

/* vis_spec_draft_batch: vis_spec_draft per sequence, one workgroup each: prompt_ids [batch][ld_prompt], prompt_len /
 * gen_start / step_ptr / n_draft [batch], tokens [batch][max_tokens], draft [batch][3].  spec.propose() on sequence b's
 * own history is the definition.  One launch. */
int vis_spec_draft_batch(const void* prompt_ids, int ld_prompt, const void* prompt_len, const void* tokens, int max_tokens,
                         const void* gen_start, const void* step_ptr, int k, int lookup_max, int lookup_min, int vocab,
                         int batch, void* draft, void* n_draft, vis_stream_t stream);

/* The speculative step under a JSON Schema (csrc/spec_schema.hip; spec.py "grammar").
 * vis_schema_mask_rows: the allow rows [rows][ld_allow] (rows 1..4) of ONE sequence's step.  Row 0 is vis_schema_mask's row
 * at *step_ptr (the same fold of tokens[position .. *step_ptr), the same "no token allowed -> EOS ids"); row r >= 1 is the
 * row of the DFA state behind draft[0 .. r), walked from row 0's state.  From the first r with r > *n_draft (clamped to
 * 0..rows-1), or whose draft[r-1] is outside [0, V), an EOS id or rejected by the walk, the rows are all-zero.  record: int32
 * [32]; words 0..3 = DFA state, error bit, position, anchored (anchored 0: the header's start state; an all-zero record is
 * a sequence whose reply starts at tokens[0]), words 8..16 the launch's counters (zero between launches).  The slot is
 * written by the workgroup that arrives last, after every workgroup has read it: *step_ptr may advance by any amount
 * between launches, and a launch repeated at the same step repeats its rows.  Only tokens[] is ever folded.  Token table,
 * DFA tables, header and capacities: vis_schema_mask's, with its argument checks (rows in the place of batch). */
int vis_schema_mask_rows(void* record, const void* tokens, int max_tokens, const void* step_ptr, const void* draft,
                         const void* n_draft, int rows, const void* tok_off, const void* tok_bytes, const void* tok_flags,
                         const void* eos_ids, int n_eos, int V, void* allow, int ld_allow, const void* header,
                         const void* trans, const void* byte_class, const void* state_flags, int cap_states,
                         int cap_classes, vis_stream_t stream);
/* vis_spec_draft_schema: the drafter that reads the schema (schema_draft.propose).  Folds tokens[position .. *step_ptr)
 * into the state of vis_schema_mask_rows' record (read only), then follows jump_tok / jump_next (int32 [cap_states]: per
 * DFA state the longest token spelling a prefix of the bytes the schema forces there, -1 = none, and the state behind it)
 * up to k (1..3) times, stopping at an entry outside [0, V) / [0, n_states).  n > 0 drafts: draft[0 .. n) and *n_draft = n;
 * none (also: error state, bad header): draft and *n_draft are left as the drafter in front wrote them.  One workgroup. */
int vis_spec_draft_schema(const void* record, const void* tokens, int max_tokens, const void* step_ptr, const void* tok_off,
                          const void* tok_bytes, const void* tok_flags, int V, const void* header, const void* trans,
                          const void* byte_class, const void* state_flags, int cap_states, int cap_classes,
                          const void* jump_tok, const void* jump_next, int k, void* draft, void* n_draft,
                          vis_stream_t stream);

/* ---- Row f2: Llama-3.2-11B-Vision ("mllama") Auditor, reference src/agents/vlm_auditor.py:81-83,:152-158 ---- */

/* Resized RGB frame -> patch rows of the tile canvas (zero padding applied to RAW pixels, then rescale/normalise;
 * TF:models/mllama/image_processing_pil_mllama.py pad/split_to_tiles_np; Conv2d feature order (c, ph, pw),
 * TF:models/mllama/modeling_mllama.py:833-840).  Row of tile t, patch (py, px): t*((tile/14)^2+1) + 1 + py*(tile/14) + px;
 * CLS rows and absent tiles are not written (the caller zero-fills). */
int vis_patchify_tiles_u8(const void* img, void* out, int H, int W, int tiles_h, int tiles_w, int tile, int ld_out,
                          const float* mean, const float* stdv, vis_stream_t stream);

/* x[i][:] += table[idx[i]][:] (bf16, f32 add): per-tile embeddings broadcast over a tile's tokens
 * (TF:models/mllama/modeling_mllama.py:102-122). */
int vis_add_rows_bf16(void* x, const void* table, const void* idx, int n, int D, int ldx, int n_table,
                      vis_stream_t stream);

/* Decode-step cross-attention over a static key/value set (TF:models/mllama/modeling_mllama.py:384-466): q [Hq*128]
 * from the q projection (per-head q_norm applied inside), k/v [Hkv][key_tokens][128], *nkeys_m1 = valid keys - 1. */
int vis_decode_cross_attn(const void* q, const void* q_norm_w, const void* k, const void* v, const void* nkeys_m1,
                          void* part_o, void* part_ml, void* out, int Hq, int Hkv, int HD, int key_tokens,
                          int nsplit, float scale, float eps, vis_stream_t stream);
/* Batch form: sequence b uses q + b * q_bs, k / v + b * kv_bs (element strides) and nkeys_m1[b]; out [batch][Hq*128]. */
int vis_decode_cross_attn_batch(const void* q, const void* q_norm_w, const void* k, const void* v,
                                const void* nkeys_m1, void* part_o, void* part_ml, void* out, int Hq, int Hkv, int HD,
                                int key_tokens, int nsplit, float scale, float eps, int batch, long long q_bs,
                                long long kv_bs, vis_stream_t stream);

/* vis_decode_cross_attn over fp8 (OCP e4m3) copies of the static keys / values (csrc/cross_attn.hip): codes uint8
 * [Hkv][key_tokens][128] and one f32 scale per (kv head, key row) [Hkv][key_tokens] for K and for V, as vis_quant_rows_fp8
 * (no norm) writes them over the bf16 rows.  key_tokens is a multiple of 64; codes and scales are 16-byte aligned.  Same split
 * plan, key range [0, *nkeys_m1 + 1) and partials as the bf16 entry; P stays f32, the V row scale rides in the weight. */
int vis_decode_cross_attn_fp8(const void* q, const void* q_norm_w, const void* k_codes, const void* k_scale,
                              const void* v_codes, const void* v_scale, const void* nkeys_m1, void* part_o, void* part_ml,
                              void* out, int Hq, int Hkv, int HD, int key_tokens, int nsplit, float scale, float eps,
                              vis_stream_t stream);
/* Batch form: sequence b uses q + b * q_bs, codes + b * kv_bs, scales + b * sc_bs (element strides) and nkeys_m1[b]. */
int vis_decode_cross_attn_fp8_batch(const void* q, const void* q_norm_w, const void* k_codes, const void* k_scale,
                                    const void* v_codes, const void* v_scale, const void* nkeys_m1, void* part_o,
                                    void* part_ml, void* out, int Hq, int Hkv, int HD, int key_tokens, int nsplit,
                                    float scale, float eps, int batch, long long q_bs, long long kv_bs, long long sc_bs,
                                    vis_stream_t stream);

/* Row f4: pixel statistics of the image-quality pre-check (src/safety/image_quality.py:42-56,:118-127): exact integer
 * sums over the RGB frame - stats[0] = sum gray, stats[1] = sum Laplacian, stats[2] = sum Laplacian^2 (int64[3]) with
 * OpenCV's published 8-bit RGB2GRAY fixed-point rule and the ksize-1 Laplacian under BORDER_REFLECT_101.
 * Parity with the reference's cv2 calls is UNPINNED (OpenCV is absent here; the reference holds no fixtures). */
int vis_image_stats_u8(const void* img, int H, int W, void* stats, vis_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VIS_HIP_H */
