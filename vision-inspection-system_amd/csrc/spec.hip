// Lossless n-gram speculative decoding of ONE greedy sequence (spec.py, DecodeStage._decode_step_spec): a step runs R = 1 + k
// rows - the current token and up to k drafted ones - through every projection in one pass over the weights
// (vis_gemv_*_rows, each row bit-identical to the single-row kernel), and keeps the longest prefix of the drafts the model
// itself would have picked.  The pieces that did not exist:
//
//  * vis_decode_attn_draft: vis_decode_attn for the R rows of one sequence.  Row r sits at position *step_ptr + r: it takes
//    that rope row, its K / V go to that cache row, it attends over keys [0, *step_ptr + r].  Three launches behind the one
//    entry point: APPEND (every row's rotated key and its value into the cache), ATTEND (the split items of every row,
//    appending nothing), COMBINE.  Row r reads the cache rows of rows 0 .. r - 1, which is why append and attend cannot share a
//    launch - the hazard that makes vis_decode_attn(batch = R, cache_bs = 0) wrong.  All three run decode_attn_split_body /
//    decode_attn_combine_body (decode_common.hip.h) with the split plan and key order of vis_decode_attn, so output row r and
//    the cache are, bit for bit, what R successive vis_decode_attn launches at advancing steps leave.  A row at a position
//    >= cache_tokens returns before it reads or writes anything.
//    (The cross layers' form of the same step, vis_decode_cross_attn_draft / _fp8_draft, lives in cross_attn.hip.)
//  * vis_spec_accept: the greedy pick of every row (vis_argmax_f32's comparison: larger value, ties to the lower id, a row
//    without a comparable logit picks id 0), the count `a` of leading drafts that equal the pick of the row in front of them,
//    and the bookkeeping of a step that produced a + 1 tokens.
//  * vis_spec_accept_sampled: the same with the Gumbel-max pick of a sampled request, row r at hash counter *step_ptr + r.
//  * vis_spec_accept_masked: either of the two with every row's pick restricted to a row of allowed ids (the speculative
//    step under a JSON Schema, spec_schema.hip).
//  * vis_spec_draft: prompt lookup - the latest earlier occurrence of the last m ids of the history (m from lookup_max down
//    to lookup_min) and the ids that followed it.  spec.propose() is its definition.
//  * vis_spec_draft_pred: the drafter of a request with a prediction (spec.propose_pred() is its definition): a cursor into
//    the caller's predicted reply, found again from the reply's tail after a deviation, with the prompt lookup above as
//    its fallback.
//  * the batch forms (spec_batch.py, the speculative step of B in-flight sequences): vis_decode_attn_draft_batch,
//    vis_spec_gather_batch, vis_spec_accept_batch, vis_spec_draft_batch - each is the single-sequence launch with the sequence
//    on the grid; sequence b's rows are packed rows b * rows .. b * rows + rows - 1 and its outputs are, bit for bit, what
//    the single-sequence entry writes for it alone.
//
// Every index that comes from device memory (*step_ptr, the draft count, the limit, lengths, token ids) is clamped before it
// forms an address.
#include "decode_common.hip.h"
#include <math.h>

#define SP_MAXLOOKUP 8

// ------------------------------------------------------------------------------------------------ vis_decode_attn_draft
template <int G>
__global__ __launch_bounds__(256) void spec_attn_append_kernel(DecAttnArgs p) {
  __shared__ DecAttnLds<G> L;
  // the split that owns the row's position (the body checks the range again, before it reads anything else)
  const int pos = max(*p.step_ptr, 0) + (int)blockIdx.y;
  if (pos >= p.cache_tokens) return;
  decode_attn_split_body<G, false, false, 1>(p, L, blockIdx.x, pos / DA_MAXKEYS, blockIdx.y,
                                             ChainCtx{nullptr, nullptr, nullptr, 0u, nullptr});
}

template <int G>
__global__ __launch_bounds__(256) void spec_attn_attend_kernel(DecAttnArgs p) {
  __shared__ DecAttnLds<G> L;
  decode_attn_split_body<G, false, false, 2>(p, L, blockIdx.x, blockIdx.y, blockIdx.z, ChainCtx{nullptr, nullptr, nullptr, 0u, nullptr});
}

__global__ __launch_bounds__(256) void spec_attn_combine_kernel(const float* __restrict__ part_o, const float* __restrict__ part_ml,
                                                                bf16_t* __restrict__ out, int nsplit,
                                                                const int* __restrict__ step_ptr, int cache_tokens) {
  if (max(*step_ptr, 0) + (int)blockIdx.y >= cache_tokens) return;     // workgroup-uniform: a row past the cache has no partials
  decode_attn_combine_body(part_o, part_ml, out, nsplit, step_ptr, cache_tokens, 1);
}

template <int G>
static void spec_attn_launch(const DecAttnArgs& p, bf16_t* out, int rows, hipStream_t stream) {
  hipLaunchKernelGGL(spec_attn_append_kernel<G>, dim3(p.Hkv, rows), dim3(256), 0, stream, p);
  hipLaunchKernelGGL(spec_attn_attend_kernel<G>, dim3(p.Hkv, p.nsplit, rows), dim3(256), 0, stream, p);
  hipLaunchKernelGGL(spec_attn_combine_kernel, dim3(p.Hq, rows), dim3(256), 0, stream, (const float*)p.part_o,
                     (const float*)p.part_ml, out, p.nsplit, p.step_ptr, p.cache_tokens);
}

extern "C" int vis_decode_attn_draft(const void* qkv, const void* cos_t, const void* sin_t, void* k_cache, void* v_cache,
                                     const void* step_ptr, void* part_o, void* part_ml, void* out, int Hq, int Hkv, int HD,
                                     int cache_tokens, int nsplit, float scale, int rows, long long qkv_ld,
                                     hipStream_t stream) {
  if (!qkv || !cos_t || !sin_t || !k_cache || !v_cache || !step_ptr || !part_o || !part_ml || !out) return VIS_ERR_ARG;
  if (rows < 1 || rows > SP_MAXROWS) return VIS_ERR_ARG;
  if (HD != 128 || Hq <= 0 || Hkv <= 0 || Hq % Hkv != 0) return VIS_ERR_ARG;
  if (qkv_ld < (long long)(Hq + 2 * Hkv) * 128 || (qkv_ld % 8)) return VIS_ERR_ARG;
  const int G = Hq / Hkv;
  if (G != 1 && G != 2 && G != 4 && G != 7 && G != 8) return VIS_ERR_ARG;  // instantiated GQA group sizes
  if (nsplit <= 0 || nsplit > 256 || cache_tokens <= 0) return VIS_ERR_ARG;
  if ((long long)nsplit * DA_MAXKEYS < cache_tokens) return VIS_ERR_ARG;  // every key must be covered
  if (((uintptr_t)k_cache | (uintptr_t)v_cache) & 15) return VIS_ERR_ARG;
  if (((uintptr_t)step_ptr | (uintptr_t)part_o | (uintptr_t)part_ml | (uintptr_t)cos_t | (uintptr_t)sin_t) & 3) return VIS_ERR_ARG;
  if (((uintptr_t)qkv | (uintptr_t)out) & 1) return VIS_ERR_ARG;
  DecAttnArgs p;
  p.qkv = (const bf16_t*)qkv; p.cos_t = (const float*)cos_t; p.sin_t = (const float*)sin_t;
  p.k_cache = (bf16_t*)k_cache; p.v_cache = (bf16_t*)v_cache; p.step_ptr = (const int*)step_ptr;
  p.part_o = (float*)part_o; p.part_ml = (float*)part_ml;
  p.Hq = Hq; p.Hkv = Hkv; p.cache_tokens = cache_tokens; p.nsplit = nsplit;
  p.scale_log2 = scale * 1.4426950408889634f;
  p.qkv_bs = qkv_ld; p.cache_bs = 0; p.tab_bs = 0;      // the rows share one cache and one pair of rope tables
  p.q_norm_w = nullptr; p.q_eps = 0.f;
  p.shared_len = 0;
  p.fork_parent = nullptr; p.fork_len = nullptr;
  da_no_parts(p);
  vis_clear_error();
  da_dispatch_g(G, [&](auto g) { spec_attn_launch<decltype(g)::value>(p, (bf16_t*)out, rows, stream); });
  return vis_check_launch();
}

// ------------------------------------------------------------------------------------------ vis_decode_attn_draft_batch
// vis_decode_attn_draft for `batch` sequences of `rows` rows each: packed row b * rows + r is row r of sequence b.  Every
// workgroup first moves the argument block to ITS sequence - projection rows, caches, rope tables, step, partials - and then
// runs the single-sequence draft item on row r: the same body, the same split plan, the same key order, so row (b, r) and
// the caches are what `rows` successive vis_decode_attn(batch) launches at advancing steps leave.  Append, attend and combine
// stay three launches for the hazard named at the head of this file (row r reads the cache rows of rows 0 .. r - 1).
__device__ __forceinline__ void sp_seq_args(DecAttnArgs& p, int b, int rows) {
  p.qkv += (long long)b * rows * p.qkv_bs;
  p.k_cache += (long long)b * p.cache_bs;
  p.v_cache += (long long)b * p.cache_bs;
  p.cos_t += (long long)b * p.tab_bs;
  p.sin_t += (long long)b * p.tab_bs;
  p.step_ptr += b;
  p.part_o += (size_t)b * rows * p.Hq * p.nsplit * 128;
  p.part_ml += (size_t)b * rows * p.Hq * p.nsplit * 2;
  p.cache_bs = 0; p.tab_bs = 0;      // from here on: the rows of ONE sequence
}

template <int G>
__global__ __launch_bounds__(256) void spec_attn_append_batch_kernel(DecAttnArgs p) {      // grid (Hkv, rows, batch)
  __shared__ DecAttnLds<G> L;
  sp_seq_args(p, blockIdx.z, gridDim.y);
  const int pos = max(*p.step_ptr, 0) + (int)blockIdx.y;
  if (pos >= p.cache_tokens) return;
  decode_attn_split_body<G, false, false, 1>(p, L, blockIdx.x, pos / DA_MAXKEYS, blockIdx.y,
                                             ChainCtx{nullptr, nullptr, nullptr, 0u, nullptr});
}

template <int G>
__global__ __launch_bounds__(256) void spec_attn_attend_batch_kernel(DecAttnArgs p, int rows) {      // grid (Hkv, nsplit, batch * rows)
  __shared__ DecAttnLds<G> L;
  const int b = (int)blockIdx.z / rows, r = (int)blockIdx.z - b * rows;
  sp_seq_args(p, b, rows);
  decode_attn_split_body<G, false, false, 2>(p, L, blockIdx.x, blockIdx.y, r, ChainCtx{nullptr, nullptr, nullptr, 0u, nullptr});
}

__global__ __launch_bounds__(256) void spec_attn_combine_batch_kernel(const float* __restrict__ part_o,      // grid (Hq, rows, batch)
                                                                      const float* __restrict__ part_ml, bf16_t* __restrict__ out,
                                                                      int nsplit, const int* __restrict__ step_ptr,
                                                                      int cache_tokens) {
  const size_t seq_rows = (size_t)blockIdx.z * gridDim.y;      // packed rows in front of this sequence's
  step_ptr += blockIdx.z;
  if (max(*step_ptr, 0) + (int)blockIdx.y >= cache_tokens) return;     // workgroup-uniform: a row past the cache has no partials
  decode_attn_combine_body(part_o + seq_rows * gridDim.x * nsplit * 128, part_ml + seq_rows * gridDim.x * nsplit * 2,
                           out + seq_rows * gridDim.x * 128, nsplit, step_ptr, cache_tokens, 1);
}

template <int G>
static void spec_attn_batch_launch(const DecAttnArgs& p, bf16_t* out, int rows, int batch, hipStream_t stream) {
  hipLaunchKernelGGL(spec_attn_append_batch_kernel<G>, dim3(p.Hkv, rows, batch), dim3(256), 0, stream, p);
  hipLaunchKernelGGL(spec_attn_attend_batch_kernel<G>, dim3(p.Hkv, p.nsplit, batch * rows), dim3(256), 0, stream, p, rows);
  hipLaunchKernelGGL(spec_attn_combine_batch_kernel, dim3(p.Hq, rows, batch), dim3(256), 0, stream, (const float*)p.part_o,
                     (const float*)p.part_ml, out, p.nsplit, p.step_ptr, p.cache_tokens);
}

extern "C" int vis_decode_attn_streams(int Hkv, int batch) {
  return (Hkv > 0 && batch > 0 && da_use_stream_form(Hkv, batch)) ? 1 : 0;
}

extern "C" int vis_decode_attn_draft_batch(const void* qkv, const void* cos_t, const void* sin_t, void* k_cache, void* v_cache,
                                           const void* step_ptr, void* part_o, void* part_ml, void* out, int Hq, int Hkv,
                                           int HD, int cache_tokens, int nsplit, float scale, int rows, int batch,
                                           long long qkv_ld, long long cache_bs, long long tab_bs, hipStream_t stream) {
  if (!qkv || !cos_t || !sin_t || !k_cache || !v_cache || !step_ptr || !part_o || !part_ml || !out) return VIS_ERR_ARG;
  if (rows < 1 || rows > SP_MAXROWS || batch < 1 || batch > 64 || batch * rows > 64) return VIS_ERR_ARG;
  if (HD != 128 || Hq <= 0 || Hkv <= 0 || Hq % Hkv != 0) return VIS_ERR_ARG;
  if (qkv_ld < (long long)(Hq + 2 * Hkv) * 128 || (qkv_ld % 8)) return VIS_ERR_ARG;
  if (cache_bs < (long long)Hkv * cache_tokens * 128 || (cache_bs % 8) || tab_bs < 0) return VIS_ERR_ARG;
  const int G = Hq / Hkv;
  if (G != 1 && G != 2 && G != 4 && G != 7 && G != 8) return VIS_ERR_ARG;  // instantiated GQA group sizes
  if (nsplit <= 0 || nsplit > 256 || cache_tokens <= 0) return VIS_ERR_ARG;
  if ((long long)nsplit * DA_MAXKEYS < cache_tokens) return VIS_ERR_ARG;  // every key must be covered
  if (((uintptr_t)k_cache | (uintptr_t)v_cache) & 15) return VIS_ERR_ARG;
  if (((uintptr_t)step_ptr | (uintptr_t)part_o | (uintptr_t)part_ml | (uintptr_t)cos_t | (uintptr_t)sin_t) & 3) return VIS_ERR_ARG;
  if (((uintptr_t)qkv | (uintptr_t)out) & 1) return VIS_ERR_ARG;
  // the plain step of these sequences would take the streaming form (another key order): nothing to be bit-identical to
  if (da_use_stream_form(Hkv, batch)) return VIS_ERR_UNSUPPORTED;
  DecAttnArgs p;
  p.qkv = (const bf16_t*)qkv; p.cos_t = (const float*)cos_t; p.sin_t = (const float*)sin_t;
  p.k_cache = (bf16_t*)k_cache; p.v_cache = (bf16_t*)v_cache; p.step_ptr = (const int*)step_ptr;
  p.part_o = (float*)part_o; p.part_ml = (float*)part_ml;
  p.Hq = Hq; p.Hkv = Hkv; p.cache_tokens = cache_tokens; p.nsplit = nsplit;
  p.scale_log2 = scale * 1.4426950408889634f;
  p.qkv_bs = qkv_ld; p.cache_bs = cache_bs; p.tab_bs = tab_bs;
  p.q_norm_w = nullptr; p.q_eps = 0.f;
  p.shared_len = 0;
  p.fork_parent = nullptr; p.fork_len = nullptr;
  da_no_parts(p);
  vis_clear_error();
  da_dispatch_g(G, [&](auto g) { spec_attn_batch_launch<decltype(g)::value>(p, (bf16_t*)out, rows, batch, stream); });
  return vis_check_launch();
}

// ------------------------------------------------------------------------------------------------------ vis_spec_accept
// vis_argmax_f32's comparison: the candidate replaces the best when it is larger, or equal with the lower id.  NaN compares
// false both ways and is never picked; the sentinel id (no comparable logit) becomes id 0 where the pick is used.
__device__ __forceinline__ void sp_better(float& best, int& bi, float v, int i) {
  if (v > best || (v == best && i < bi)) { best = v; bi = i; }
}

__device__ __forceinline__ void sp_wave_best(float& best, int& bi) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    sp_better(best, bi, ov, oi);
  }
}

// stage 1: grid (nb, rows), 256 threads: workgroup x of row r leaves (max, lowest id) over its ids in ws[r][x]
__global__ __launch_bounds__(256) void spec_pick_kernel(const float* __restrict__ logits, int V, int ld,
                                                        float* __restrict__ bval, int* __restrict__ bidx) {
  const int tid = threadIdx.x, row = blockIdx.y;
  const float* __restrict__ x = logits + (size_t)row * ld;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int i = blockIdx.x * 256 + tid; i < V; i += gridDim.x * 256) sp_better(best, bi, x[i], i);
  sp_wave_best(best, bi);
  __shared__ float sv[4];
  __shared__ int si[4];
  if ((tid & 63) == 0) { sv[tid >> 6] = best; si[tid >> 6] = bi; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w) sp_better(best, bi, sv[w], si[w]);
    bval[row * 256 + blockIdx.x] = best;
    bidx[row * 256 + blockIdx.x] = bi;
  }
}

// stage 2: one workgroup of 256 threads, wave r merges row r; then lane 0 of wave 0 does the step's bookkeeping
// (the body: vis_spec_accept_batch runs it once per sequence, one workgroup each)
__device__ __forceinline__ void spec_accept_body(const float* __restrict__ bval, const int* __restrict__ bidx, int nb, int rows,
                                                 const int* __restrict__ draft, const int* __restrict__ n_draft,
                                                 const int* __restrict__ limit, int* __restrict__ tokens, int max_tokens,
                                                 int* __restrict__ cur_token, int* __restrict__ step_ptr,
                                                 int* __restrict__ counters) {
  __shared__ int pick[SP_MAXROWS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (wave < rows) {
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = lane; i < nb; i += 64) sp_better(best, bi, bval[wave * 256 + i], bidx[wave * 256 + i]);
    sp_wave_best(best, bi);
    if (lane == 0) pick[wave] = (bi == 0x7fffffff) ? 0 : bi;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const int st = *step_ptr;
  const int lim = min(*limit, max_tokens - 1);
  if (st < 0 || st > lim) return;     // the request has all its tokens: a step issued ahead of the poll changes nothing
  const int d = min(max(*n_draft, 0), rows - 1);
  int a = 0;
  while (a < d && draft[a] == pick[a]) ++a;
  a = min(a, lim - st);               // tokens[st .. st + a] are written: st + a <= limit
  for (int r = 0; r <= a; ++r) tokens[st + r] = pick[r];
  *cur_token = pick[a];
  *step_ptr = st + a + 1;
  counters[0] += 1;
  counters[1] += d;
  counters[2] += a;
}

__global__ __launch_bounds__(256) void spec_accept_kernel(const float* __restrict__ bval, const int* __restrict__ bidx, int nb,
                                                          int rows, const int* __restrict__ draft,
                                                          const int* __restrict__ n_draft, const int* __restrict__ limit,
                                                          int* __restrict__ tokens, int max_tokens, int* __restrict__ cur_token,
                                                          int* __restrict__ step_ptr, int* __restrict__ counters) {
  spec_accept_body(bval, bidx, nb, rows, draft, n_draft, limit, tokens, max_tokens, cur_token, step_ptr, counters);
}

extern "C" int vis_spec_accept(const void* logits, int V, int ld_logits, int rows, const void* draft, const void* n_draft,
                               const void* limit, void* ws_val, void* ws_idx, void* tokens, int max_tokens, void* cur_token,
                               void* step_ptr, void* counters, hipStream_t stream) {
  if (!logits || !draft || !n_draft || !limit || !ws_val || !ws_idx || !tokens || !cur_token || !step_ptr || !counters)
    return VIS_ERR_ARG;
  if (V <= 0 || rows < 1 || rows > SP_MAXROWS || ld_logits < V || max_tokens <= 0) return VIS_ERR_ARG;
  if (((uintptr_t)logits | (uintptr_t)draft | (uintptr_t)n_draft | (uintptr_t)limit | (uintptr_t)ws_val | (uintptr_t)ws_idx |
       (uintptr_t)tokens | (uintptr_t)cur_token | (uintptr_t)step_ptr | (uintptr_t)counters) & 3)
    return VIS_ERR_ARG;
  const int nb = min(256, (V + 255) / 256);
  vis_clear_error();
  hipLaunchKernelGGL(spec_pick_kernel, dim3(nb, rows), dim3(256), 0, stream, (const float*)logits, V, ld_logits,
                     (float*)ws_val, (int*)ws_idx);
  hipLaunchKernelGGL(spec_accept_kernel, dim3(1), dim3(256), 0, stream, (const float*)ws_val, (const int*)ws_idx, nb, rows,
                     (const int*)draft, (const int*)n_draft, (const int*)limit, (int*)tokens, max_tokens, (int*)cur_token,
                     (int*)step_ptr, (int*)counters);
  return vis_check_launch();
}

// ---------------------------------------------------------------------------------------------- vis_spec_accept_sampled
// vis_spec_accept with the SAMPLED pick of every row: row r perturbs id i with gumbel_noise(seed, *step_ptr + r, i) - the
// hash counter the plain loop has when it picks from these logits - in argmax_stage1_body's source expression and under its
// tie rule, so row r's pick is the token vis_argmax_f32 stores for that row at step *step_ptr + r, bit for bit.  inv_temp and
// seed come from device memory (8 bytes, read at run time): one captured step serves every temperature and seed.  An
// inv_temp that is not > 0 (0, negative, NaN) leaves the logits alone: vis_spec_accept's picks.  The step only feeds the
// hash, never an address.  Stage 2 is spec_accept_kernel itself.
struct SpSampleParams {
  float inv_temp;
  unsigned seed;
};

__global__ __launch_bounds__(256) void spec_pick_sampled_kernel(const float* __restrict__ logits, int V, int ld,
                                                                const int* __restrict__ step_ptr,
                                                                const SpSampleParams* __restrict__ params,
                                                                float* __restrict__ bval, int* __restrict__ bidx) {
  const int tid = threadIdx.x, row = blockIdx.y;
  const float* __restrict__ x = logits + (size_t)row * ld;
  const float inv_temp = params->inv_temp;
  const unsigned seed = params->seed;
  const unsigned step = (unsigned)*step_ptr + (unsigned)row;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int i = blockIdx.x * 256 + tid; i < V; i += gridDim.x * 256) {
    float v = x[i];
    if (inv_temp > 0.f) v = v * inv_temp + gumbel_noise(seed, step, (unsigned)i);
    sp_better(best, bi, v, i);
  }
  sp_wave_best(best, bi);
  __shared__ float sv[4];
  __shared__ int si[4];
  if ((tid & 63) == 0) { sv[tid >> 6] = best; si[tid >> 6] = bi; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w) sp_better(best, bi, sv[w], si[w]);
    bval[row * 256 + blockIdx.x] = best;
    bidx[row * 256 + blockIdx.x] = bi;
  }
}

extern "C" int vis_spec_accept_sampled(const void* logits, int V, int ld_logits, int rows, const void* draft, const void* n_draft,
                                       const void* limit, void* ws_val, void* ws_idx, void* tokens, int max_tokens,
                                       void* cur_token, void* step_ptr, void* counters, const void* params, hipStream_t stream) {
  if (!logits || !draft || !n_draft || !limit || !ws_val || !ws_idx || !tokens || !cur_token || !step_ptr || !counters || !params)
    return VIS_ERR_ARG;
  if (V <= 0 || rows < 1 || rows > SP_MAXROWS || ld_logits < V || max_tokens <= 0) return VIS_ERR_ARG;
  if (((uintptr_t)logits | (uintptr_t)draft | (uintptr_t)n_draft | (uintptr_t)limit | (uintptr_t)ws_val | (uintptr_t)ws_idx |
       (uintptr_t)tokens | (uintptr_t)cur_token | (uintptr_t)step_ptr | (uintptr_t)counters | (uintptr_t)params) & 3)
    return VIS_ERR_ARG;
  const int nb = min(256, (V + 255) / 256);
  vis_clear_error();
  hipLaunchKernelGGL(spec_pick_sampled_kernel, dim3(nb, rows), dim3(256), 0, stream, (const float*)logits, V, ld_logits,
                     (const int*)step_ptr, (const SpSampleParams*)params, (float*)ws_val, (int*)ws_idx);
  hipLaunchKernelGGL(spec_accept_kernel, dim3(1), dim3(256), 0, stream, (const float*)ws_val, (const int*)ws_idx, nb, rows,
                     (const int*)draft, (const int*)n_draft, (const int*)limit, (int*)tokens, max_tokens, (int*)cur_token,
                     (int*)step_ptr, (int*)counters);
  return vis_check_launch();
}

// ------------------------------------------------------------------------------------------------ vis_spec_accept_batch
// vis_spec_accept / vis_spec_accept_sampled per sequence.  Stage 1, grid (nb, rows, batch): logits row b * rows + r with
// spec_pick_kernel's loop (params null) or spec_pick_sampled_kernel's - sequence b's own inverse temperature and seed, hash
// counter step[b] + r - into ws[(b * rows + r) * 256 + x]: the comparison is a total order, so the pick is the single-sequence
// entry's whatever the workgroup count.  Stage 2, grid (batch): spec_accept_body on sequence b's rows and state.
__global__ __launch_bounds__(256) void spec_pick_batch_kernel(const float* __restrict__ logits, int V, int ld,
                                                              const int* __restrict__ step_ptr,
                                                              const SpSampleParams* __restrict__ params,
                                                              float* __restrict__ bval, int* __restrict__ bidx) {
  const int tid = threadIdx.x, row = blockIdx.z * gridDim.y + blockIdx.y;
  const float* __restrict__ x = logits + (size_t)row * ld;
  const float inv_temp = params ? params[blockIdx.z].inv_temp : 0.f;
  const unsigned seed = params ? params[blockIdx.z].seed : 0u;
  const unsigned step = (unsigned)step_ptr[blockIdx.z] + (unsigned)blockIdx.y;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int i = blockIdx.x * 256 + tid; i < V; i += gridDim.x * 256) {
    float v = x[i];
    if (inv_temp > 0.f) v = v * inv_temp + gumbel_noise(seed, step, (unsigned)i);
    sp_better(best, bi, v, i);
  }
  sp_wave_best(best, bi);
  __shared__ float sv[4];
  __shared__ int si[4];
  if ((tid & 63) == 0) { sv[tid >> 6] = best; si[tid >> 6] = bi; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w) sp_better(best, bi, sv[w], si[w]);
    bval[row * 256 + blockIdx.x] = best;
    bidx[row * 256 + blockIdx.x] = bi;
  }
}

__global__ __launch_bounds__(256) void spec_accept_batch_kernel(const float* __restrict__ bval, const int* __restrict__ bidx,
                                                                int nb, int rows, const int* __restrict__ draft,
                                                                const int* __restrict__ n_draft, const int* __restrict__ limit,
                                                                int* __restrict__ tokens, int max_tokens,
                                                                int* __restrict__ cur_token, int* __restrict__ step_ptr,
                                                                int* __restrict__ counters) {
  const int b = blockIdx.x;
  spec_accept_body(bval + (size_t)b * rows * 256, bidx + (size_t)b * rows * 256, nb, rows, draft + b * (SP_MAXROWS - 1),
                   n_draft + b, limit + b, tokens + (size_t)b * max_tokens, max_tokens, cur_token + b, step_ptr + b,
                   counters + b * 3);
}

extern "C" int vis_spec_accept_batch(const void* logits, int V, int ld_logits, int rows, int batch, const void* draft,
                                     const void* n_draft, const void* limit, void* ws_val, void* ws_idx, void* tokens,
                                     int max_tokens, void* cur_token, void* step_ptr, void* counters, const void* params,
                                     hipStream_t stream) {
  if (!logits || !draft || !n_draft || !limit || !ws_val || !ws_idx || !tokens || !cur_token || !step_ptr || !counters)
    return VIS_ERR_ARG;
  if (V <= 0 || rows < 1 || rows > SP_MAXROWS || batch < 1 || batch > 64 || batch * rows > 64 || ld_logits < V || max_tokens <= 0)
    return VIS_ERR_ARG;
  if (((uintptr_t)logits | (uintptr_t)draft | (uintptr_t)n_draft | (uintptr_t)limit | (uintptr_t)ws_val | (uintptr_t)ws_idx |
       (uintptr_t)tokens | (uintptr_t)cur_token | (uintptr_t)step_ptr | (uintptr_t)counters | (uintptr_t)params) & 3)
    return VIS_ERR_ARG;
  const int nb = min(256, (V + 255) / 256);
  vis_clear_error();
  hipLaunchKernelGGL(spec_pick_batch_kernel, dim3(nb, rows, batch), dim3(256), 0, stream, (const float*)logits, V, ld_logits,
                     (const int*)step_ptr, (const SpSampleParams*)params, (float*)ws_val, (int*)ws_idx);
  hipLaunchKernelGGL(spec_accept_batch_kernel, dim3(batch), dim3(256), 0, stream, (const float*)ws_val, (const int*)ws_idx, nb,
                     rows, (const int*)draft, (const int*)n_draft, (const int*)limit, (int*)tokens, max_tokens, (int*)cur_token,
                     (int*)step_ptr, (int*)counters);
  return vis_check_launch();
}

// ------------------------------------------------------------------------------------------------ vis_spec_gather_batch
// The input rows of a batched speculative step: out[b * rows + r][:] = table[id][:] with id = cur[b] for r = 0 and
// draft[b][r - 1] behind it (vis_gather_rows' copy and clamp; drafts past n_draft[b] are whatever the drafter left - their
// rows are computed and never accepted).  One wave per row.
__global__ __launch_bounds__(256) void spec_gather_batch_kernel(const bf16_t* __restrict__ table, const int* __restrict__ cur,
                                                                const int* __restrict__ draft, bf16_t* __restrict__ out,
                                                                int n, int rows, int D, int n_table) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= n) return;
  const int b = row / rows, r = row - b * rows;
  int id = r ? draft[b * (SP_MAXROWS - 1) + r - 1] : cur[b];
  id = id < 0 ? 0 : (id >= n_table ? n_table - 1 : id);
  const bf16_t* src = table + (size_t)id * D;
  bf16_t* dst = out + (size_t)row * D;
  for (int c = lane; c < (D >> 3); c += 64) *(u32x4*)(dst + c * 8) = *(const u32x4*)(src + c * 8);
}

extern "C" int vis_spec_gather_batch(const void* table, const void* cur_token, const void* draft, void* out, int rows, int batch,
                                     int D, int n_table, hipStream_t stream) {
  if (!table || !cur_token || !draft || !out) return VIS_ERR_ARG;
  if (rows < 1 || rows > SP_MAXROWS || batch < 1 || batch > 64 || batch * rows > 64 || D <= 0 || D % 8 != 0 || n_table <= 0)
    return VIS_ERR_ARG;
  if ((((uintptr_t)table | (uintptr_t)out) & 15) || (((uintptr_t)cur_token | (uintptr_t)draft) & 3)) return VIS_ERR_ARG;
  const int n = batch * rows;
  vis_clear_error();
  hipLaunchKernelGGL(spec_gather_batch_kernel, dim3((n + 3) / 4), dim3(256), 0, stream, (const bf16_t*)table,
                     (const int*)cur_token, (const int*)draft, (bf16_t*)out, n, rows, D, n_table);
  return vis_check_launch();
}

// ----------------------------------------------------------------------------------------------- vis_spec_accept_masked
// vis_spec_accept / vis_spec_accept_sampled with row r's pick restricted to the ids whose bit is set in allow + r * ld_allow
// (vis_schema_mask_rows' rows): argmax_stage1_body<MASK>'s loop - the mask test in front of the same expression, the same
// tie rule - so row r's pick is the token vis_argmax_masked_f32 (batch 1) stores for that row with *step_ptr = step + r, bit
// for bit; a row without an allowed id picks 0.  params null: the greedy pick.  Stage 2 is spec_accept_kernel itself.
__global__ __launch_bounds__(256) void spec_pick_masked_kernel(const float* __restrict__ logits, int V, int ld,
                                                               const int* __restrict__ step_ptr,
                                                               const SpSampleParams* __restrict__ params,
                                                               const unsigned long long* __restrict__ allow, int ld_allow,
                                                               float* __restrict__ bval, int* __restrict__ bidx) {
  const int tid = threadIdx.x, row = blockIdx.y;
  const float* __restrict__ x = logits + (size_t)row * ld;
  const unsigned long long* __restrict__ al = allow + (size_t)row * ld_allow;
  const float inv_temp = params ? params->inv_temp : 0.f;
  const unsigned seed = params ? params->seed : 0u;
  const unsigned step = (unsigned)*step_ptr + (unsigned)row;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int i = blockIdx.x * 256 + tid; i < V; i += gridDim.x * 256) {
    if (!((al[i >> 6] >> (i & 63)) & 1ull)) continue;
    float v = x[i];
    if (inv_temp > 0.f) v = v * inv_temp + gumbel_noise(seed, step, (unsigned)i);
    sp_better(best, bi, v, i);
  }
  sp_wave_best(best, bi);
  __shared__ float sv[4];
  __shared__ int si[4];
  if ((tid & 63) == 0) { sv[tid >> 6] = best; si[tid >> 6] = bi; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w) sp_better(best, bi, sv[w], si[w]);
    bval[row * 256 + blockIdx.x] = best;
    bidx[row * 256 + blockIdx.x] = bi;
  }
}

extern "C" int vis_spec_accept_masked(const void* logits, int V, int ld_logits, int rows, const void* draft, const void* n_draft,
                                      const void* limit, void* ws_val, void* ws_idx, void* tokens, int max_tokens,
                                      void* cur_token, void* step_ptr, void* counters, const void* params, const void* allow,
                                      int ld_allow, hipStream_t stream) {
  if (!logits || !draft || !n_draft || !limit || !ws_val || !ws_idx || !tokens || !cur_token || !step_ptr || !counters || !allow)
    return VIS_ERR_ARG;
  if (V <= 0 || rows < 1 || rows > SP_MAXROWS || ld_logits < V || max_tokens <= 0) return VIS_ERR_ARG;
  if (ld_allow < (V + 63) / 64 || ((uintptr_t)allow & 7)) return VIS_ERR_ARG;
  if (((uintptr_t)logits | (uintptr_t)draft | (uintptr_t)n_draft | (uintptr_t)limit | (uintptr_t)ws_val | (uintptr_t)ws_idx |
       (uintptr_t)tokens | (uintptr_t)cur_token | (uintptr_t)step_ptr | (uintptr_t)counters | (uintptr_t)params) & 3)
    return VIS_ERR_ARG;
  const int nb = min(256, (V + 255) / 256);
  vis_clear_error();
  hipLaunchKernelGGL(spec_pick_masked_kernel, dim3(nb, rows), dim3(256), 0, stream, (const float*)logits, V, ld_logits,
                     (const int*)step_ptr, (const SpSampleParams*)params, (const unsigned long long*)allow, ld_allow,
                     (float*)ws_val, (int*)ws_idx);
  hipLaunchKernelGGL(spec_accept_kernel, dim3(1), dim3(256), 0, stream, (const float*)ws_val, (const int*)ws_idx, nb, rows,
                     (const int*)draft, (const int*)n_draft, (const int*)limit, (int*)tokens, max_tokens, (int*)cur_token,
                     (int*)step_ptr, (int*)counters);
  return vis_check_launch();
}

// ------------------------------------------------------------------------------------------------------- vis_spec_draft
// History h = prompt[0 .. plen) followed by tokens[gen0 .. step), length L (vis_ban_f32's reading of the same rows).  For m =
// lookup_max down to lookup_min with L > m: the largest j < L - m with h[j .. j + m) == h[L - m .. L); the first m that has
// one wins: draft = h[j + m .. min(j + m + k, L)), *n_draft its length.  No match: *n_draft = 0 and draft is left alone.
// One workgroup: 256 lanes take the candidate starts j in strides, the largest matching j is reduced through LDS.
// The lookup itself, shared with vis_spec_draft_pred (its fallback): returns d (uniform) and writes draft[0 .. d); d = 0 leaves
// draft alone.  ``wbest``: four ints of LDS.  Every lane of the workgroup calls it.
__device__ __forceinline__ int sp_prompt_lookup(const int* __restrict__ prompt, int P, const int* __restrict__ gn, int L, int k,
                                                int lookup_max, int lookup_min, int vocab, int* __restrict__ draft, int* wbest) {
  const int tid = threadIdx.x;
#define SP_H(i) ((i) < P ? prompt[(i)] : gn[(i) - P])
  for (int m = lookup_max; m >= lookup_min; --m) {
    if (L <= m) continue;     // (uniform) no room for the pattern and one id after an earlier copy of it
    int tail[SP_MAXLOOKUP];
#pragma unroll
    for (int i = 0; i < SP_MAXLOOKUP; ++i) tail[i] = (i < m) ? SP_H(L - m + i) : 0;
    int best = -1;
    for (int j = tid; j < L - m; j += 256) {
      bool match = true;
#pragma unroll
      for (int i = 0; i < SP_MAXLOOKUP; ++i)
        if (i < m && match) match = SP_H(j + i) == tail[i];
      if (match) best = j;      // ascending j per lane: the last one stays
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best = max(best, __shfl_xor(best, o, 64));
    __syncthreads();            // the previous round's readers are through
    if ((tid & 63) == 0) wbest[tid >> 6] = best;
    __syncthreads();
    best = max(max(wbest[0], wbest[1]), max(wbest[2], wbest[3]));
    if (best >= 0) {            // uniform
      const int from = best + m, d = min(k, L - from);
      if (tid < d) draft[tid] = min(max(SP_H(from + tid), 0), vocab - 1);
      return d;
    }
  }
#undef SP_H
  return 0;
}

// (the body: vis_spec_draft_batch runs it once per sequence, one workgroup each)
__device__ __forceinline__ void spec_draft_body(const int* __restrict__ prompt, int ld_prompt, const int* __restrict__ plen,
                                                const int* __restrict__ tokens, int max_tokens, const int* __restrict__ gen0,
                                                const int* __restrict__ step_ptr, int k, int lookup_max, int lookup_min, int vocab,
                                                int* __restrict__ draft, int* __restrict__ n_draft) {
  __shared__ int wbest[4];
  const int P = min(max(*plen, 0), ld_prompt);
  const int end = min(max(*step_ptr, 0), max_tokens);
  const int s0 = min(max(*gen0, 0), end);
  const int d = sp_prompt_lookup(prompt, P, tokens + s0, P + (end - s0), k, lookup_max, lookup_min, vocab, draft, wbest);
  if (threadIdx.x == 0) *n_draft = d;
}

__global__ __launch_bounds__(256) void spec_draft_kernel(const int* __restrict__ prompt, int ld_prompt, const int* __restrict__ plen,
                                                         const int* __restrict__ tokens, int max_tokens,
                                                         const int* __restrict__ gen0, const int* __restrict__ step_ptr, int k,
                                                         int lookup_max, int lookup_min, int vocab, int* __restrict__ draft,
                                                         int* __restrict__ n_draft) {
  spec_draft_body(prompt, ld_prompt, plen, tokens, max_tokens, gen0, step_ptr, k, lookup_max, lookup_min, vocab, draft, n_draft);
}

// vis_spec_draft per sequence: workgroup b reads prompt row b, token row b and its own counters, writes draft[b][0 .. d)
__global__ __launch_bounds__(256) void spec_draft_batch_kernel(const int* __restrict__ prompt, int ld_prompt,
                                                               const int* __restrict__ plen, const int* __restrict__ tokens,
                                                               int max_tokens, const int* __restrict__ gen0,
                                                               const int* __restrict__ step_ptr, int k, int lookup_max,
                                                               int lookup_min, int vocab, int* __restrict__ draft,
                                                               int* __restrict__ n_draft) {
  const int b = blockIdx.x;
  spec_draft_body(prompt + (size_t)b * ld_prompt, ld_prompt, plen + b, tokens + (size_t)b * max_tokens, max_tokens, gen0 + b,
                  step_ptr + b, k, lookup_max, lookup_min, vocab, draft + b * (SP_MAXROWS - 1), n_draft + b);
}

extern "C" int vis_spec_draft(const void* prompt_ids, int ld_prompt, const void* prompt_len, const void* tokens, int max_tokens,
                              const void* gen_start, const void* step_ptr, int k, int lookup_max, int lookup_min, int vocab,
                              void* draft, void* n_draft, hipStream_t stream) {
  if (!prompt_ids || !prompt_len || !tokens || !gen_start || !step_ptr || !draft || !n_draft) return VIS_ERR_ARG;
  if (ld_prompt <= 0 || max_tokens <= 0 || vocab <= 0 || k < 1 || k > SP_MAXROWS - 1) return VIS_ERR_ARG;
  if (lookup_max < 1 || lookup_max > SP_MAXLOOKUP || lookup_min < 1 || lookup_min > lookup_max) return VIS_ERR_ARG;
  if (((uintptr_t)prompt_ids | (uintptr_t)prompt_len | (uintptr_t)tokens | (uintptr_t)gen_start | (uintptr_t)step_ptr |
       (uintptr_t)draft | (uintptr_t)n_draft) & 3)
    return VIS_ERR_ARG;
  vis_clear_error();
  hipLaunchKernelGGL(spec_draft_kernel, dim3(1), dim3(256), 0, stream, (const int*)prompt_ids, ld_prompt, (const int*)prompt_len,
                     (const int*)tokens, max_tokens, (const int*)gen_start, (const int*)step_ptr, k, lookup_max, lookup_min,
                     vocab, (int*)draft, (int*)n_draft);
  return vis_check_launch();
}

extern "C" int vis_spec_draft_batch(const void* prompt_ids, int ld_prompt, const void* prompt_len, const void* tokens,
                                    int max_tokens, const void* gen_start, const void* step_ptr, int k, int lookup_max,
                                    int lookup_min, int vocab, int batch, void* draft, void* n_draft, hipStream_t stream) {
  if (!prompt_ids || !prompt_len || !tokens || !gen_start || !step_ptr || !draft || !n_draft) return VIS_ERR_ARG;
  if (ld_prompt <= 0 || max_tokens <= 0 || vocab <= 0 || k < 1 || k > SP_MAXROWS - 1 || batch < 1 || batch > 64) return VIS_ERR_ARG;
  if (lookup_max < 1 || lookup_max > SP_MAXLOOKUP || lookup_min < 1 || lookup_min > lookup_max) return VIS_ERR_ARG;
  if (((uintptr_t)prompt_ids | (uintptr_t)prompt_len | (uintptr_t)tokens | (uintptr_t)gen_start | (uintptr_t)step_ptr |
       (uintptr_t)draft | (uintptr_t)n_draft) & 3)
    return VIS_ERR_ARG;
  vis_clear_error();
  hipLaunchKernelGGL(spec_draft_batch_kernel, dim3(batch), dim3(256), 0, stream, (const int*)prompt_ids, ld_prompt,
                     (const int*)prompt_len, (const int*)tokens, max_tokens, (const int*)gen_start, (const int*)step_ptr, k,
                     lookup_max, lookup_min, vocab, (int*)draft, (int*)n_draft);
  return vis_check_launch();
}

// -------------------------------------------------------------------------------------------------- vis_spec_draft_pred
// One spec.propose_pred() call on device memory: the drafter of a request that came with a prediction (OpenAI's Predicted
// Outputs).  A cursor walks the prediction while the reply follows it; a reply token that differs loses the cursor, and the
// last lookup_max .. lookup_min ids of the reply find it again - forward of where it was lost first, else the nearest place
// behind.  While the cursor is lost or past the prediction's end the draft is vis_spec_draft's prompt lookup.
// state: cursor, last, seen, src, n_out, accepted, rejected (spec.PredState).  One workgroup, one pass over the prediction:
// every lane keeps, per match length, the smallest candidate >= last and the largest one < last of its stride; the
// longest match length is reduced first (a maximum), then that length's two candidates (a minimum and a maximum), so the
// result does not depend on which lane saw what.
#define SP_ST_INTS 7

__device__ __forceinline__ int sp_block_max(int v, int* lds) {      // lds: four ints nobody else uses
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  return max(max(lds[0], lds[1]), max(lds[2], lds[3]));
}

__global__ __launch_bounds__(256) void spec_draft_pred_kernel(const int* __restrict__ prompt, int ld_prompt,
                                                              const int* __restrict__ plen, const int* __restrict__ tokens,
                                                              int max_tokens, const int* __restrict__ gen0,
                                                              const int* __restrict__ step_ptr, int k, int lookup_max,
                                                              int lookup_min, int vocab, const int* __restrict__ pred, int ld_pred,
                                                              const int* __restrict__ pred_len, int* __restrict__ state,
                                                              int* __restrict__ draft, int* __restrict__ n_draft) {
  __shared__ int wbest[4], rmax[4], rfwd[4], rbwd[4];
  const int tid = threadIdx.x;
  const int PL = min(max(*plen, 0), ld_prompt);
  const int end = min(max(*step_ptr, 0), max_tokens);
  const int s0 = min(max(*gen0, 0), end);
  const int Lr = end - s0;                  // the reply so far, the newest pick included
  const int* __restrict__ gn = tokens + s0;
  const int P = min(max(*pred_len, 0), ld_pred);
  int cursor = state[0], last = state[1];
  const int seen = min(max(state[2], 0), Lr), src = state[3], n_out = max(state[4], 0);
  int acc = state[5], rej = state[6];
  __syncthreads();                          // every lane holds the state before lane 0 replaces it
  // 1. what the accept step kept of the drafts of the previous call (a step behind the limit brought nothing: no count)
  if (Lr > seen && src == 2) {
    const int a = min(Lr - seen - 1, n_out);
    acc += a;
    rej += n_out - a;
  }
  // 2. the cursor follows the new tokens (every lane, the same few compares)
  for (int i = seen; i < Lr && cursor >= 0; ++i) {
    if (cursor < P && pred[cursor] == gn[i]) ++cursor;
    else { last = cursor; cursor = -1; }
  }
  // 3. lost: the longest tail of the reply that stands in the prediction with an id behind it
  if (cursor < 0 && P > 0) {                // uniform
    const int mtop = min(lookup_max, Lr);
    int tail[SP_MAXLOOKUP], fmin[SP_MAXLOOKUP], bmax[SP_MAXLOOKUP];
#pragma unroll
    for (int i = 0; i < SP_MAXLOOKUP; ++i) {
      tail[i] = (i < mtop) ? gn[Lr - 1 - i] : 0;      // backwards: tail[0] is the newest id
      fmin[i] = 0x7fffffff;
      bmax[i] = -1;
    }
    int mine = 0;
    for (int e = 1 + tid; e < P; e += 256) {           // candidate: pred[e] would be drafted next
      const int cap = min(mtop, e);
      int ml = 0;
#pragma unroll
      for (int i = 0; i < SP_MAXLOOKUP; ++i)
        if (i == ml && i < cap && pred[e - 1 - i] == tail[i]) ml = i + 1;
      mine = max(mine, ml);
#pragma unroll
      for (int i = 0; i < SP_MAXLOOKUP; ++i)
        if (i < ml) {
          if (e >= last) fmin[i] = min(fmin[i], e);
          else bmax[i] = max(bmax[i], e);
        }
    }
    const int M = sp_block_max(mine, rmax);            // uniform: the first m of the definition that has a candidate
    if (M >= lookup_min) {
      int f = 0x7fffffff, b = -1;
#pragma unroll
      for (int i = 0; i < SP_MAXLOOKUP; ++i)
        if (i == M - 1) { f = fmin[i]; b = bmax[i]; }
      f = -sp_block_max(-f, rfwd);                     // the minimum (f >= 1, so -f has no overflow)
      b = sp_block_max(b, rbwd);
      cursor = (f != 0x7fffffff) ? f : b;
    }
  }
  // 4. the draft
  int d, nsrc;
  if (cursor >= 0 && cursor < P) {
    d = min(k, P - cursor);
    if (tid < d) draft[tid] = min(max(pred[cursor + tid], 0), vocab - 1);
    nsrc = 2;
  } else {
    d = sp_prompt_lookup(prompt, PL, gn, PL + Lr, k, lookup_max, lookup_min, vocab, draft, wbest);
    nsrc = d > 0 ? 1 : 0;
  }
  if (tid == 0) {
    *n_draft = d;
    state[0] = cursor; state[1] = last; state[2] = Lr; state[3] = nsrc; state[4] = d; state[5] = acc; state[6] = rej;
  }
}

extern "C" int vis_spec_draft_pred(const void* prompt_ids, int ld_prompt, const void* prompt_len, const void* tokens,
                                   int max_tokens, const void* gen_start, const void* step_ptr, int k, int lookup_max,
                                   int lookup_min, int vocab, const void* pred_ids, int ld_pred, const void* pred_len, void* state,
                                   void* draft, void* n_draft, hipStream_t stream) {
  if (!prompt_ids || !prompt_len || !tokens || !gen_start || !step_ptr || !pred_ids || !pred_len || !state || !draft || !n_draft)
    return VIS_ERR_ARG;
  if (ld_prompt <= 0 || ld_pred <= 0 || max_tokens <= 0 || vocab <= 0 || k < 1 || k > SP_MAXROWS - 1) return VIS_ERR_ARG;
  if (lookup_max < 1 || lookup_max > SP_MAXLOOKUP || lookup_min < 1 || lookup_min > lookup_max) return VIS_ERR_ARG;
  if (((uintptr_t)prompt_ids | (uintptr_t)prompt_len | (uintptr_t)tokens | (uintptr_t)gen_start | (uintptr_t)step_ptr |
       (uintptr_t)pred_ids | (uintptr_t)pred_len | (uintptr_t)state | (uintptr_t)draft | (uintptr_t)n_draft) & 3)
    return VIS_ERR_ARG;
  vis_clear_error();
  hipLaunchKernelGGL(spec_draft_pred_kernel, dim3(1), dim3(256), 0, stream, (const int*)prompt_ids, ld_prompt,
                     (const int*)prompt_len, (const int*)tokens, max_tokens, (const int*)gen_start, (const int*)step_ptr, k,
                     lookup_max, lookup_min, vocab, (const int*)pred_ids, ld_pred, (const int*)pred_len, (int*)state, (int*)draft,
                     (int*)n_draft);
  return vis_check_launch();
}
